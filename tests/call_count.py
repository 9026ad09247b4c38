"""Counting the calls of C entry points from a test: the library's functions are looked up by attribute at call time, so a shim
set on the loaded library sees every call under its entry's name."""
from flowtron_amd import _lib as L


def count_calls(monkeypatch, names):
    lib = L.lib()
    calls = {n: 0 for n in names}
    for name in names:
        fn = getattr(lib, name)

        def shim(*a, _fn=fn, _n=name):
            calls[_n] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, shim)
    return calls
