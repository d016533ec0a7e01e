"""Writes tests/golden/python_api_surface.json: what `import wordpiece_amd` shows a caller — the public names, the public
methods of Vocab with their signatures, every ctypes.Structure with its fields, the public int constants and the tables
ABI_SYMBOLS, QUALITY_RULES, QUALITY_SIGNALS, DEFAULT_RESERVED.  Needs no built library (lib() loads it on first use).
tests/test_python_api_surface.py computes the same through surface() and compares; docstrings are not part of it.
Run it on purpose only: when a change means to move the public surface."""
import ctypes
import inspect
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "python_api_surface.json")


def _field(name, ctype):
    """(name, ctypes type name, array length or None)"""
    if isinstance(ctype, type) and issubclass(ctype, ctypes.Array):
        return [name, ctype._type_.__name__, ctype._length_]
    return [name, ctype.__name__, None]


def surface(W):
    """the public surface of the package module W as JSON-ready data"""
    public = {n: getattr(W, n) for n in dir(W) if not n.startswith("_") and not isinstance(getattr(W, n), types.ModuleType)}
    methods = {}
    for n, m in sorted(vars(W.Vocab).items()):
        if n.startswith("_"):
            continue
        if isinstance(m, property):
            methods[n] = "property"
        else:
            methods[n] = str(inspect.signature(getattr(W.Vocab, n)))
    structs = {n: [_field(*f) for f in x._fields_] for n, x in sorted(public.items())
               if isinstance(x, type) and issubclass(x, ctypes.Structure)}
    constants = {n: x for n, x in sorted(public.items()) if isinstance(x, int) and not isinstance(x, bool)}
    return {"names": sorted(public), "vocab_methods": methods, "structures": structs, "constants": constants,
            "ABI_SYMBOLS": list(W.ABI_SYMBOLS), "QUALITY_RULES": list(W.QUALITY_RULES), "QUALITY_SIGNALS": list(W.QUALITY_SIGNALS),
            "DEFAULT_RESERVED": list(W.DEFAULT_RESERVED)}


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import wordpiece_amd as W
    with open(PATH, "w") as f:
        json.dump(surface(W), f, ensure_ascii=True, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
