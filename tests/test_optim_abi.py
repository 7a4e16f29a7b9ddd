"""AdamW update with per-tensor step counters (mmdit_adamw_step_dlr_pt) at the ABI level.  No GPU needed.

The entry point lives in a header of its own, include/mmdit_hip_optim.h, and in the binding's _OPTIM_SIGNATURES table: the versioned core ABI (58
entry points, MMDIT_ABI_VERSION 10) and the other headers do not move.  The device code is adamw_kernel's own (one flag in its constants), so no
kernel is added; ClipAdamW.step_clipped launches it with the flat tensor of its `step` scalars."""
import ctypes
import inspect
import os
import re

NAME = "mmdit_adamw_step_dlr_pt"


def _lib():
    import sd3_amd  # noqa: F401
    from sd3_amd import _lib
    return _lib


def _prototype(txt, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"no prototype of {name}"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_declared_in_the_optim_header_only():
    L = _lib()
    assert L.declared_optim_symbols() == [NAME] and set(L._OPTIM_SIGNATURES) == {NAME}
    for table in (L._SIGNATURES, L._EXT_SIGNATURES, L._HD128_SIGNATURES, L._ROPE3_SIGNATURES, L._QKHALF_SIGNATURES, L._TEXTLOSS_SIGNATURES, L._COS2_SIGNATURES,
                  L._FP8PAD_SIGNATURES, L._MXPAD_SIGNATURES):
        assert NAME not in table
    for path in (L.HEADER_PATH, L.HEADER_EXT_PATH, L.HEADER_HD128_PATH, L.HEADER_ROPE3_PATH, L.HEADER_QKHALF_PATH, L.HEADER_TEXTLOSS_PATH, L.HEADER_COS2_PATH,
                 L.HEADER_FP8PAD_PATH, L.HEADER_MXPAD_PATH):
        with open(path) as f:
            assert NAME not in f.read(), path
    with open(L.HEADER_OPTIM_PATH) as f:
        txt = f.read()
    assert '#include "mmdit_hip.h"' in txt and "step_counts[chunk_tensor[c]] + 1" in txt


def test_the_core_abi_does_not_move():
    L = _lib()
    assert len(L.declared_symbols()) == 58 and L.ABI_VERSION == 10 and set(L._SIGNATURES) == set(L.declared_symbols())
    with open(L.HEADER_PATH) as f:
        assert re.search(r"#define\s+MMDIT_ABI_VERSION\s+10\b", f.read())
    assert L.declared_ext_symbols() == ["mmdit_attn_fwd_e4m3"] and set(L._EXT_SIGNATURES) == {"mmdit_attn_fwd_e4m3"}


def test_signature_equals_the_prototype_and_its_single_counter_namesake():
    L = _lib()
    with open(L.HEADER_OPTIM_PATH) as f:
        txt = f.read()
    with open(L.HEADER_PATH) as f:
        core = f.read()
    args = _prototype(txt, NAME)
    assert [a.replace("step_counts", "step_count") for a in args] == _prototype(core, "mmdit_adamw_step_dlr")
    argtypes, restype = L._OPTIM_SIGNATURES[NAME]
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert restype is i and argtypes == [vp, vp, vp, i, vp, vp, vp, d, d, d, d, vp] and len(argtypes) == len(args)


def test_bound_and_exported():
    L = _lib()
    assert hasattr(ctypes.CDLL(L.LIB_PATH), NAME)
    fn = getattr(L.lib(), NAME)
    assert fn.argtypes == L._OPTIM_SIGNATURES[NAME][0] and fn.restype is L._OPTIM_SIGNATURES[NAME][1]
    assert L.lib().mmdit_abi_version() == 10


def test_build_lists_the_header_and_the_kernel_is_shared():
    import importlib.util
    L = _lib()
    spec = importlib.util.spec_from_file_location("_mmdit_build_optim", os.path.join(os.path.dirname(L.LIB_PATH), "build.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    assert os.path.samefile(B.HEADER_OPTIM, L.HEADER_OPTIM_PATH) and "optim.hip" in B.SOURCES
    with open(os.path.join(B.CSRC, "optim.hip")) as f:
        txt = f.read()
    assert "mmdit_hip_optim.h" in txt and len(re.findall(r'extern "C" int ' + NAME + r"\(", txt)) == 1
    assert len(re.findall(r"__global__[^;{]*\bvoid adamw_kernel\(", txt)) == 1


def test_step_clipped_launches_the_per_tensor_form():
    import sd3_amd  # noqa: F401
    from sd3_amd import optim
    src = inspect.getsource(optim.ClipAdamW.step_clipped)
    assert "mmdit_adamw_step_dlr_pt(" in src and "vp(steps_flat)" in src and "mmdit_adamw_step_dlr(" not in src
