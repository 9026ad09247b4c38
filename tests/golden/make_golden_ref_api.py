"""The reference's interface as data, so the CPU interface tests run without the reference checked out:
    python tests/golden/make_golden_ref_api.py
  ref_api.json   config.json's model_config and the train_config keys FlowtronLoss is built from (train.py:221, :236-238);
                 the parameter names of every constructor / method the scripts call (flowtron.py classes, radam.RAdam,
                 data.Data / DataCollate, the distributed.py entry points); and the names train.py / inference.py import
                 from the five drop-in modules; train.py's prepare_dataloaders: its parameters and the keywords of the
                 Data / DataCollate / DataLoader calls it makes.  Names and literal values only: no source text."""
import ast
import importlib.util
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import refshim  # noqa: E402

DROPINS = ("flowtron", "data", "radam", "distributed", "audio_processing")
CALLS = (("Flowtron", ("__init__", "forward", "infer")), ("FlowtronLoss", ("__init__", "forward")), ("AR_Step", ("__init__",)),
         ("Encoder", ("__init__",)), ("Attention", ("__init__",)))


def _sig(fn):
    return [p.name for p in inspect.signature(fn).parameters.values()]


def _ast(name):
    return ast.parse(open(os.path.join(refshim.REF_DIR, name)).read())


def _def_args(tree, cls, fn):
    body = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls][0].body if cls else tree.body
    return [a.arg for a in [n for n in body if isinstance(n, ast.FunctionDef) and n.name == fn][0].args.args]


def _calls(fn_node):
    """{callee: {keyword: literal value or None (an expression)}} of the named calls inside a function"""
    out = {}
    for n in ast.walk(fn_node):
        if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.keywords:
            kw = {}
            for k in n.keywords:
                if k.arg is None:
                    continue
                try:
                    kw[k.arg] = ast.literal_eval(k.value)
                except ValueError:
                    kw[k.arg] = None
            out.setdefault(n.func.id, {}).update(kw)
    return out


def prepare_dataloaders_spec(tree):
    """parameter names of prepare_dataloaders and the keywords (literal values) of the calls it makes"""
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "prepare_dataloaders"][0]
    return {"args": [a.arg for a in fn.args.args], "calls": _calls(fn)}


def main():
    assert refshim.available(), "needs the reference checkout"
    R = refshim.load()
    cfg = json.load(open(os.path.join(refshim.REF_DIR, "config.json")))
    spec = importlib.util.spec_from_file_location("_ref_radam", os.path.join(refshim.REF_DIR, "radam.py"))
    rr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rr)
    data_t, dist_t = _ast("data.py"), _ast("distributed.py")
    imports = {}
    for script in ("train.py", "inference.py"):
        names = {}
        for node in _ast(script).body:
            if isinstance(node, ast.ImportFrom) and node.module in DROPINS:
                names.setdefault(node.module, []).extend(a.name for a in node.names)
        imports[script] = names
    out = {
        "config": {"model_config": cfg["model_config"],
                   "train_config": {k: cfg["train_config"][k] for k in ("sigma", "gate_loss", "use_ctc_loss", "ctc_loss_weight",
                                                                         "blank_logprob")}},
        "signatures": {"%s.%s" % (cls, m): _sig(getattr(getattr(R, cls), m)) for cls, meths in CALLS for m in meths},
        "radam_init": _sig(rr.RAdam.__init__),
        "data_init": _def_args(data_t, "Data", "__init__"),
        "datacollate_init": _def_args(data_t, "DataCollate", "__init__"),
        "distributed": {f: _def_args(dist_t, None, f) for f in ("init_distributed", "apply_gradient_allreduce", "reduce_tensor")},
        "script_imports": imports,
        "train_prepare_dataloaders": prepare_dataloaders_spec(_ast("train.py")),
    }
    with open(os.path.join(HERE, "ref_api.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out["script_imports"]))


if __name__ == "__main__":
    main()
