"""The planner of the grouped weight-gradient GEMMs (ft_gemm_img_group_plan: a pure host function, no launch, no device access) on
the problem list of a training step at the benchmark's shape: two flows, 19 200 compact rows of capacity, plus the encoder's dense
gradients.  The pointers are made-up addresses: the planner looks at them for alignment and for overlap of the C matrices only."""
import pytest

from flowtron_amd import _lib as L

SLOTS = {256: 512, 128: 1024}                    # workgroup slots of the chip per tile height (2 and 4 workgroups on each of 256 CUs)
CAP = 19232                                      # compact rows of capacity of the step (T * B + B)
FLOW = [(4096, 1664), (4096, 1024), (4096, 1024), (4096, 1024), (4096, 1024), (1024, 1024), (1024, 1024), (640, 1024), (4096, 80), (160, 1024)]
ENCODER = [(1536, 1536, 3200), (512, 2560, 3200), (2048, 512, 3200)]


def problem(M, N, K, c_addr, ldc=None, compact=0, split=True, beta=1.0):
    up = lambda v: (v + 255) // 256 * 256
    return L.GemmImgArgs(0x100000, 0x200000, c_addr, None, M, N, K, up(M), up(N), ldc or N, 1, 1, 1.0, beta, 0, L.GEMM_SPLITK if split else 0,
                         None, 0x300000 if compact else None, compact, 0, None, None, None, 0, None)


def plan(probs):
    arr = (L.GemmImgArgs * len(probs))(*probs)
    out = (L.GemmImgGroupPlan * len(probs))()
    L.check(L.lib().ft_gemm_img_group_plan(arr, len(probs), out), "ft_gemm_img_group_plan")
    return list(out)


def step_problems():
    probs, addr = [], 0x10000000
    for _ in range(2):
        for M, N in FLOW:
            probs.append(problem(M, N, CAP, addr, compact=2))
            addr += M * N * 4 + 256
    for M, N, K in ENCODER:
        probs.append(problem(M, N, K, addr))
        addr += M * N * 4 + 256
    return probs


def test_every_tile_and_k_step_is_covered_by_exactly_one_unit():
    probs = step_problems()
    pl = plan(probs)
    for launch in sorted(set(p.launch for p in pl)):
        owner = {}
        for i, (a, p) in enumerate(zip(probs, pl)):
            if p.launch != launch:
                continue
            assert p.tile_rows == (256 if a.M >= 512 else 128)
            assert p.tiles == -(-a.M // p.tile_rows) * -(-a.N // 128)
            nk = -(-a.K // 32)
            assert p.ksteps == -(-nk // p.splits) and (p.splits - 1) * p.ksteps < nk, "an empty k-slice"
            seen = {}
            for u in range(p.tiles * p.splits):
                assert owner.setdefault(p.unit0 + u, i) == i, "unit %d belongs to two problems" % (p.unit0 + u)
                tile, sl = u % p.tiles, u // p.tiles
                for k in range(sl * p.ksteps, min(nk, (sl + 1) * p.ksteps)):
                    assert seen.setdefault((tile, k), u) == u
            assert len(seen) == p.tiles * nk, "problem %d: %d of %d (tile, k-step) pairs covered" % (i, len(seen), p.tiles * nk)
        assert sorted(owner) == list(range(len(owner))), "the units of launch %d leave a gap" % launch


def test_unit_lengths_of_a_launch_are_near_equal_and_the_longest_come_first():
    probs = step_problems()
    pl = plan(probs)
    for launch in sorted(set(p.launch for p in pl)):
        mine = sorted((p for p in pl if p.launch == launch), key=lambda p: p.unit0)
        lens = [p.ksteps for p in mine]
        assert lens == sorted(lens, reverse=True), "longest units first: %s" % lens
        # a problem's slices can only be whole: with s slices of length l, one slice more or fewer changes l by about l / s -- that is
        # the granularity the lengths of a launch may differ by (a problem that may not split at all is as long as it is)
        split = [p for p in mine if p.splits > 1]
        if split:
            gran = max(-(-p.ksteps // p.splits) for p in split)
            assert max(p.ksteps for p in split) - min(p.ksteps for p in split) <= gran, [(p.ksteps, p.splits) for p in split]
            assert max(lens) <= max(p.ksteps for p in split) + gran, lens
        units = sum(p.tiles * p.splits for p in mine)
        # as few slices as fill the slots: never more than one unit per k-slice of 16 steps, and the big launch has whole rounds' worth
        if launch == 0:
            assert units >= 2 * SLOTS[256]
            assert all(p.splits <= 4 for p in mine), [p.splits for p in mine]


def test_overlapping_outputs_are_atomic_and_disjoint_windows_plain():
    K = 96                                            # one k-slice each: only the overlap decides
    base = 0x40000000
    probs = [problem(300, 130, K, base, split=False),                                     # 0: alone -> plain
             problem(300, 130, K, base + 0x100000, split=False),                          # 1 and 2: the same C
             problem(300, 130, K, base + 0x100000, split=False),
             problem(160, 96, K, base + 0x200000, ldc=256, split=False),                  # 3 and 4: column windows 0..95 and 96..255 of one matrix
             problem(160, 160, K, base + 0x200000 + 96 * 4, ldc=256, split=False),
             problem(160, 96, K, base + 0x300000, ldc=256, split=False),                  # 5 and 6: windows 0..95 and 64..159 overlap
             problem(160, 96, K, base + 0x300000 + 64 * 4, ldc=256, split=False),
             problem(64, 64, K, base + 0x400000, ldc=64, split=False),                    # 7 and 8: rows 0..63 and 32..95 of one matrix
             problem(64, 64, K, base + 0x400000 + 32 * 64 * 4, ldc=64, split=False)]
    pl = plan(probs)
    assert [p.atomics for p in pl] == [0, 1, 1, 0, 0, 1, 1, 1, 1]
    assert all(p.splits == 1 for p in pl)
    # a split problem adds with atomics whoever its neighbours are
    pl = plan([problem(300, 130, 4160, base)])
    assert pl[0].splits > 1 and pl[0].atomics == 1


def test_refuses_what_is_not_a_weight_gradient_problem():
    lib = L.lib()
    out = (L.GemmImgGroupPlan * 1)()
    bad = problem(300, 130, 96, 0x40000000)
    bad.b_kmajor = 0
    assert lib.ft_gemm_img_group_plan((L.GemmImgArgs * 1)(bad), 1, out) != 0
    bad = problem(300, 130, 96, 0x40000000, beta=0.5)
    assert lib.ft_gemm_img_group_plan((L.GemmImgArgs * 1)(bad), 1, out) != 0
    many = [problem(64, 64, 96, 0x40000000 + i * 0x10000) for i in range(L.GEMM_GROUP_MAX + 1)]
    outm = (L.GemmImgGroupPlan * len(many))()
    assert lib.ft_gemm_img_group_plan((L.GemmImgArgs * len(many))(*many), len(many), outm) != 0
    assert lib.ft_gemm_img_group_plan((L.GemmImgArgs * len(many))(*many), L.GEMM_GROUP_MAX, outm) == 0
