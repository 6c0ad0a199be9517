"""CPU suite: the C-ABI shared object loads and exports every symbol include/fumi_hip.h declares (no compute)."""
import ctypes
import os
import re

from conftest import ROOT


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "fumi_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fumi_hip_\w+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from fumi_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = ctypes.CDLL(hip.LIB_PATH)
    declared = _declared_symbols()
    assert declared, "no declarations parsed"
    for s in declared:
        assert hasattr(L, s), f"{s} declared in include/fumi_hip.h but not exported"
    assert sorted(hip.SYMBOLS) == declared, "fumi_amd/hip.py binds a different symbol set than the header declares"


def _c_class(arg):
    """Class of one declared argument: p pointer (anything with * and fumi_stream_t), i4 / i8 integers, f4 float, f8 double."""
    words = arg.replace("*", " * ").split()
    if "*" in words or "fumi_stream_t" in words:
        return "p"
    for word, cls in (("double", "f8"), ("float", "f4"), ("int64_t", "i8"), ("uint64_t", "i8"), ("size_t", "i8"), ("long", "i8"),
                      ("int", "i4"), ("unsigned", "i4")):
        if word in words:
            return cls
    raise AssertionError(f"argument {arg!r} of include/fumi_hip.h has a type this test does not know")


def _ctypes_class(t):
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, (ctypes._Pointer, ctypes.Array)):
        return "p"
    if t in (ctypes.c_float, ctypes.c_double):
        return "f%d" % ctypes.sizeof(t)
    return "i%d" % ctypes.sizeof(t)


def _prototypes():
    src = open(os.path.join(ROOT, "include", "fumi_hip.h")).read()
    src = re.sub(r"//.*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    out = {}
    for name, args in re.findall(r"\b(fumi_hip_\w+)\s*\(([^)]*)\)\s*;", src):
        out[name] = [_c_class(a) for a in args.split(",") if a.strip() not in ("", "void")]
    return out


def test_argtypes_agree_with_the_header_argument_by_argument():
    """A miscounted argtypes list is silent stack corruption: every bound function takes what its prototype declares, in count and
    in class (pointer, 4-byte integer, 8-byte integer, float, double)."""
    from fumi_amd import hip
    L = hip.lib()
    protos = _prototypes()
    assert sorted(protos) == _declared_symbols(), "a declaration of include/fumi_hip.h was not parsed as a prototype"
    assert sum(1 for a in protos.values() if a) >= 91
    assert {"fumi_hip_hyper_plan", "fumi_hip_hyper_plan_query"} <= set(protos)
    for name, want in protos.items():
        argtypes = getattr(L, name).argtypes
        if not want:
            assert not argtypes, f"{name} takes no arguments"
            continue
        assert argtypes is not None, f"{name}: fumi_amd/hip.py sets no argtypes"
        got = [_ctypes_class(t) for t in argtypes]
        assert len(got) == len(want), f"{name}: {len(got)} argtypes, the header declares {len(want)} arguments"
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, f"{name}: argument {i} is bound as {g}, the header declares {w}"


def test_strerror_and_version_without_gpu():
    from fumi_amd import hip
    L = hip.lib()
    assert L.fumi_hip_version() >= 100
    assert L.fumi_hip_strerror(0) == b"ok"
    assert L.fumi_hip_strerror(-1) == b"invalid argument"


def test_product_path_fails_loudly_without_gpu_tensors():
    import pytest
    import torch
    from fumi_amd import hip
    with pytest.raises(hip.FumiHipError):
        hip.Workspace("cpu")
    with pytest.raises(hip.FumiHipError):
        hip.glove_bag(None, torch.zeros(1, 2, dtype=torch.int64), torch.zeros(3, 4), 0)


def test_hyper_plan_entry_points_without_gpu():
    """fumi_hip_hyper_plan copies at most n entries and refuses a NULL array; the query is host arithmetic: it answers without a GPU
    and refuses, before anything else, what the step itself refuses."""
    from fumi_amd import hip
    L = hip.lib()
    v = (ctypes.c_int * 9)(*([-7] * 9))
    assert L.fumi_hip_hyper_plan(v, 3) == 0 and list(v)[3:] == [-7] * 6
    assert L.fumi_hip_hyper_plan(None, 7) != 0 and L.fumi_hip_hyper_plan(v, -1) != 0
    assert len(hip.HYPER_PLAN_KEYS) == 7 and set(hip.hyper_plan()) == set(hip.HYPER_PLAN_KEYS)
    p = hip.hyper_plan_query(2, 5, 5, 5, 24, [8, 16], 20, 64, 1, want_text_grad=True)
    assert p == dict(fwd_form=3, fwd_inst=20, nrb=1, nch=1, bwd_form=3, bwd_dpasses=1, text_grad=1)
    hid = (ctypes.c_int * 1)(0)
    assert L.fumi_hip_hyper_plan_query(2, 5, 5, 5, 24, 0, hid, 20, 64, 1, 1, 0, v, 7) != 0          # no hidden layer
    assert L.fumi_hip_hyper_plan_query(2, 5, 5, 5, 24, 1, hid, 0, 64, 1, 1, 0, v, 7) != 0           # Dt = 0
    assert L.fumi_hip_hyper_plan_query(2, 5, 5, 5, 24, 1, None, 20, 64, 1, 1, 0, v, 7) != 0
