"""The reference's own scripts against the drop-in modules, on CPU (`-m "not gpu"`), from data this repository holds
(VERDICT r1 "next" 6).  tests/golden/ref_api.json records, from the reference checkout (tests/golden/make_golden_ref_api.py),
the names train.py / inference.py import from the five drop-in modules and the parameter names of everything they call:

  * HERE: every name the scripts import resolves to this repo's drop-in (`flowtron`, `data`, `radam`, `distributed`,
    `audio_processing` from the repository root), and train.py's `prepare_dataloaders` as tests/ref_loop.py restates it
    (train.py:56-81) runs against the drop-in `Data` / `DataCollate` through a real DataLoader worker on a synthetic data set;
    the call signatures the scripts rely on are compared with the reference's;
  * on the GPU box (tests/test_gpu_train_loop.py): tests/ref_loop.py restates train.py:205-377 / inference.py:40-71 call for
    call and drives the drop-ins through fp32, bf16 and fp16 + GradScaler iterations, a checkpoint, a resume and inference.
"""
import inspect
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_api.json")))

_DRIVER = r'''
import importlib, json, os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
imports = json.loads(%(imports)r)
mods, missing = {}, []
for script, by_mod in imports.items():
    for name, attrs in by_mod.items():
        m = importlib.import_module(name)
        mods[name] = os.path.abspath(m.__file__)
        missing += ["%%s: %%s.%%s" %% (script, name, a) for a in attrs if not hasattr(m, a)]
import ref_fixture
import ref_loop
cfg_path, cfg = ref_fixture.make_config(%(tmp)r, train_overrides={"batch_size": 3}, data_overrides={"p_arpabet": 1.0})
loader, valset, collate = ref_loop.prepare_dataloaders(cfg["data_config"], 1, cfg["train_config"]["batch_size"],
                                                       ref_loop.grapheme_frontend)
shapes = []
for i, batch in enumerate(loader):                      # DataLoader(num_workers=1, collate_fn=DataCollate): train.py:77-80
    mel, spk, txt, in_lens, out_lens, gate, prior = batch
    shapes.append(dict(mel=type(mel).__name__, audio=list(mel.audio.shape), n_samples=mel.n_samples.tolist(), spk=spk.tolist(),
                       txt=list(txt.shape), in_lens=in_lens.tolist(), out_lens=out_lens.tolist(), gate=list(gate.shape),
                       gate_sum=gate.sum(1).tolist(), prior=type(prior).__name__))
    if i == 1:
        break
print("RESULT " + json.dumps(dict(mods=mods, missing=missing, shapes=shapes, n_val=len(valset), bs=cfg["train_config"]["batch_size"],
                                  uses=dict(use_attn_prior=bool(collate.use_attn_prior)))))
'''


def test_script_imports_resolve_to_the_dropins_and_the_train_py_dataloader_runs(tmp_path):
    code = _DRIVER % dict(root=ROOT, tmp=str(tmp_path), imports=json.dumps(API["script_imports"]))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert set(API["script_imports"]["train.py"]) == {"flowtron", "data", "radam", "distributed"}
    assert not res["missing"], res["missing"]
    for name in res["mods"]:
        assert res["mods"][name] == os.path.join(ROOT, name + ".py"), res["mods"]
    assert res["bs"] == 3 and res["uses"]["use_attn_prior"]
    assert len(res["shapes"]) == 2
    for s in res["shapes"]:
        assert s["mel"] == "DeferredMel" and s["prior"] == "DeferredPrior"
        assert s["audio"][0] == 3 and s["txt"][0] == 3 and s["gate"][0] == 3
        assert s["in_lens"] == sorted(s["in_lens"], reverse=True)                      # data.py:200-202
        assert s["out_lens"] == [n // 256 + 1 for n in s["n_samples"]]                 # audio_processing.py:221-225
        assert s["gate"][1] == max(s["out_lens"])
        assert s["gate_sum"] == [float(s["gate"][1] - t + 1) for t in s["out_lens"]]   # ones from frame len-1 on (data.py:235)


def _sig(fn):
    return [p.name for p in inspect.signature(fn).parameters.values()]


def test_call_signatures_match_the_reference():
    """every constructor / method the scripts call on the drop-ins has the reference's parameter names, in order."""
    sys.path.insert(0, ROOT)
    import flowtron
    for key, ref in API["signatures"].items():
        cls, m = key.split(".")
        mine = _sig(getattr(getattr(flowtron, cls), m))
        assert mine[:len(ref)] == ref or (cls, m) == ("AR_Step", "forward"), (cls, m, ref, mine)
    assert len(API["signatures"]) == 8
    import radam
    assert _sig(radam.RAdam.__init__)[:6] == API["radam_init"]
    import data
    assert _sig(data.Data.__init__)[:len(API["data_init"])] == API["data_init"]
    assert _sig(data.DataCollate.__init__)[:3] == API["datacollate_init"]
    for fn in ("get_text", "get_speaker_id", "get_mel", "create_speaker_lookup_table", "__getitem__", "__len__"):
        assert hasattr(data.Data, fn), fn
    import distributed
    assert sorted(API["distributed"]) == ["apply_gradient_allreduce", "init_distributed", "reduce_tensor"]
    for name, args in API["distributed"].items():
        assert _sig(getattr(distributed, name))[:len(args)] == args, name


def test_ref_loop_prepare_dataloaders_restates_train_py():
    """tests/ref_loop.py's prepare_dataloaders (the one the test above and the GPU training-loop tests drive) against the reference
    train.py's, as tests/golden/ref_api.json records it: the same leading parameters, and every keyword train.py passes to Data /
    DataCollate / DataLoader passed here too, with the same value wherever train.py writes a literal (num_workers=1, drop_last ...)."""
    import ast
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_golden_ref_api import prepare_dataloaders_spec
    ref = API["train_prepare_dataloaders"]
    mine = prepare_dataloaders_spec(ast.parse(open(os.path.join(ROOT, "tests", "ref_loop.py")).read()))
    assert mine["args"][:len(ref["args"])] == ref["args"], (mine["args"], ref["args"])
    assert set(ref["calls"]) == {"Data", "DataCollate", "DataLoader"}
    for callee, kws in ref["calls"].items():
        assert callee in mine["calls"], callee
        for k, v in kws.items():
            assert k in mine["calls"][callee], (callee, k)
            if v is not None:
                assert mine["calls"][callee][k] == v, (callee, k, mine["calls"][callee][k], v)
