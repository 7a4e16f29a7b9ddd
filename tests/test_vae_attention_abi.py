"""C ABI of the VAE mid-block attention kernel (csrc/vae_attn.hip): mmdit_vae_attn_fwd is declared in include/mmdit_hip.h, bound in
_lib._SIGNATURES with the prototype's argument list, and exported by the built library.  No GPU needed."""
import ctypes
import re

NAME = "mmdit_vae_attn_fwd"


def _lib():
    import sd3_amd  # noqa: F401
    from sd3_amd import _lib
    return _lib


def test_declared_in_header():
    L = _lib()
    assert NAME in L.declared_symbols()
    with open(L.HEADER_PATH) as f:
        txt = f.read()
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, "no prototype"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const void* Q", "const void* K", "const void* V", "int ld", "int batch", "int tokens", "int C", "float scale", "void* O_bf16",
                    "mmdit_stream_t stream"]
    assert "#define MMDIT_ABI_VERSION 10" in txt and L.ABI_VERSION == 10      # the version this binding mirrors (mmdit_vae_attn_fwd itself came as a new symbol, without a bump)


def test_bound_with_the_prototype_types():
    L = _lib()
    argtypes, restype = L._SIGNATURES[NAME]
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert argtypes == [vp, vp, vp, i, i, i, i, f, vp, vp] and restype is i


def test_exported_by_the_built_library():
    L = _lib()
    lib = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(lib, NAME)
    assert getattr(L.lib(), NAME).argtypes == L._SIGNATURES[NAME][0]
