"""(-m gpu) The inner loops of attention.hip against float64 (tests/attn_ref64.py, that module's own bounds), at the smallest shapes
that reach each of them: the forward score loop is instantiated per number of active 32-key groups of a key pass (NJ = 1 .. 4), per
form (product / sum) and per tile kind (general / uniform); the backward key loop walks runs of product-form keys and leaves a run
for one sum-form key at a time.  Each case asserts from its own inputs, by the kernel's rule, that the path it names is taken.

LENS puts one utterance at either edge of every NJ in the first key pass (160 = a second pass with NJ 1): with T 40 every utterance
has a full and a ragged query tile."""
import pytest
import torch

import attn_ref64 as R
from test_gpu_attention_f64 import check_attention, env, make_attention, run_attention  # noqa: F401  (env: the fixture)

pytestmark = pytest.mark.gpu
LENS = [160, 129, 128, 97, 96, 65, 64, 33, 32, 1]
T, LK = 40, 160


def batch(A, prior, seed):
    return make_attention(T, len(LENS), LK, A, seed=seed, prior=prior, lens=torch.tensor(LENS))


def nj_of(length, key_pass=0):
    """the kernel's count of active 32-key groups of a 128-key pass"""
    return min(4, -(-(length - 128 * key_pass) // 32))


def test_lens_cover_every_nj():
    assert sorted({nj_of(n) for n in LENS}) == [1, 2, 3, 4]
    assert [nj_of(n, 1) for n in LENS if n > 128] == [1, 1]
    for nj in (1, 2, 3):                                         # both edges of each count below four
        assert 32 * nj in LENS and 32 * nj + 1 in LENS


def case_product(A, prior):
    """A 640: ten full a-chunks; A 72: one full chunk and a tail of 8"""
    c = batch(A, prior, seed=A + prior)
    assert not bool(R.sum_form_rows(c["Q"]).any()) and not bool(R.sum_form_keys(c["K"], c["lens"]).any())
    return c


def case_uniform():
    """tile 0 of every utterance has bit-identical query rows (one score row is evaluated and copied), tile 1 has not"""
    c = batch(192, True, seed=7)
    c["Q"][0:32] = c["Q"][0:1]
    assert bool((c["Q"][0:32] == c["Q"][0]).all()) and not bool((c["Q"][32:] == c["Q"][32]).all())
    return c


def case_sum_form():
    """one |q| above 20.8 in a-chunk 1 of tile 0 (general) and of tile 1 made uniform: the forward takes the sum form for that chunk
    at every NJ, on both tile kinds; the backward takes it for every key of the wave that owns a-chunk 1"""
    c = batch(192, True, seed=8)
    c["Q"][32:] = c["Q"][32:33]
    c["Q"][5, :, 70] = 21.0
    c["Q"][32:, :, 70] = -21.0
    rows = R.sum_form_rows(c["Q"])
    assert bool(rows[5].all()) and bool(rows[32:].all()) and int(rows[:32].sum()) == len(LENS)
    assert not bool(((R.C2 * c["Q"][:, :, :64]).abs() > R.EXP_SAFE).any())          # a-chunk 0 stays in the product form
    return c


def case_runs():
    """one sum-form key in the middle of an utterance (key 5 of utterance 3, a-chunk 0), product-form keys on either side: the
    backward's wave of a-chunk 0 leaves its run for that key and starts another; a sum-form key FIRST (utterance 4) and LAST
    (utterance 5); two in a row (utterance 6)"""
    c = batch(128, False, seed=9)
    K = c["K"]
    K[5, 3, 10] = 21.5
    K[0, 4, 11] = -21.5
    K[LENS[5] - 1, 5, 12] = 21.5
    K[8, 6, 13] = 21.5
    K[9, 6, 14] = -21.5
    keys = R.sum_form_keys(K, c["lens"])
    assert [int(keys[:, b].sum()) for b in range(len(LENS))] == [0, 0, 0, 1, 1, 1, 2, 0, 0, 0]
    assert bool(keys[5, 3]) and not bool(keys[4, 3]) and not bool(keys[6, 3])
    assert not bool(R.sum_form_rows(c["Q"]).any())
    return c


def case_single_tile():
    """B 1, T 32: every dK and dv word receives exactly one atomic"""
    return make_attention(32, 1, 40, 640, seed=11, prior=True, lens=torch.tensor([40]))


def run_twice(env, c, temp):
    L, ops = env
    d = {k: (t.cuda().contiguous() if torch.is_tensor(t) else t) for k, t in c.items()}
    return [run_attention(L, d["Q"], d["K"], d["v"], d["lens"], d["prior"], temp, d["dattn"], d["dlp"]) for _ in range(2)]


@pytest.mark.parametrize("A", [640, 72])
@pytest.mark.parametrize("prior", [True, False])
def test_every_nj_product_form(env, A, prior):
    check_attention(env, case_product(A, prior), 0.9, "NJ 1-4, A=%d%s" % (A, ", prior" if prior else ""), sens=("key",))


def test_every_nj_uniform_tile(env):
    check_attention(env, case_uniform(), 1.1, "NJ 1-4, uniform tile")


def test_every_nj_sum_form(env):
    check_attention(env, case_sum_form(), 0.9, "NJ 1-4, sum form")


def test_backward_run_structure(env):
    check_attention(env, case_runs(), 1.0, "backward runs", sens=("shift",))


def test_forward_is_deterministic(env):
    a, b = run_twice(env, case_product(640, True), 0.9)
    for k in ("attn", "logprob", "p_save", "de", "dQ"):
        assert torch.equal(a[k], b[k]), k


def test_single_tile_backward_is_deterministic(env):
    c = case_single_tile()
    a, b = run_twice(env, c, 1.0)
    for k in ("dQ", "dK", "dv"):
        assert torch.equal(a[k], b[k]), k
    check_attention(env, c, 1.0, "B1 T32")
