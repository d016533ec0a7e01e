"""The public surface of the Python wrapper against tests/golden/python_api_surface.json (written by
tests/golden/make_python_api_surface.py): names, Vocab's method signatures and defaults, the layouts of the ctypes
structures, the int constants and the public tables.  No GPU and no built library are needed."""
import importlib.util
import json
import os

import wordpiece_amd as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _maker():
    spec = importlib.util.spec_from_file_location("make_python_api_surface", os.path.join(GOLDEN, "make_python_api_surface.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MAKER = _maker()
with open(MAKER.PATH) as f:
    FIXTURE = json.load(f)
NOW = json.loads(json.dumps(MAKER.surface(W)))  # (through JSON: tuples become lists, as in the fixture)


def test_fixture_has_every_part():
    assert sorted(FIXTURE) == ["ABI_SYMBOLS", "DEFAULT_RESERVED", "QUALITY_RULES", "QUALITY_SIGNALS", "constants", "names",
                               "structures", "vocab_methods"]
    # (117 names with the five modules that leak into the namespace, which the fixture leaves out; 81 methods and unk_id)
    assert len(FIXTURE["names"]) >= 112 and len(FIXTURE["vocab_methods"]) >= 82 and len(FIXTURE["structures"]) >= 41
    for leaked in ("C", "np", "os", "math", "weakref"):
        assert leaked not in FIXTURE["names"]


def test_public_names():
    assert NOW["names"] == FIXTURE["names"]


def test_vocab_method_signatures():
    assert sorted(NOW["vocab_methods"]) == sorted(FIXTURE["vocab_methods"])
    moved = {k: (FIXTURE["vocab_methods"][k], v) for k, v in NOW["vocab_methods"].items() if v != FIXTURE["vocab_methods"][k]}
    assert not moved, moved


def test_structure_layouts():
    assert sorted(NOW["structures"]) == sorted(FIXTURE["structures"])
    moved = [k for k, v in NOW["structures"].items() if v != FIXTURE["structures"][k]]
    assert not moved, moved


def test_constants():
    assert NOW["constants"] == FIXTURE["constants"]


def test_tables():
    for k in ("ABI_SYMBOLS", "QUALITY_RULES", "QUALITY_SIGNALS", "DEFAULT_RESERVED"):
        assert NOW[k] == FIXTURE[k], k
