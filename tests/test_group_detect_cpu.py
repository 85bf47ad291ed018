"""agx_group_detect_enqueue / agx_group_detect_fetch without a GPU: the library exports both, and their argument checks answer
before any HIP call."""
import ctypes as C

AGX_ERR_ARG = -1


def _lib():
    from aprilgrid_rs_amd import _ffi
    return _ffi.lib()


def test_the_library_exports_both_entry_points():
    lib = _lib()
    assert hasattr(lib, "agx_group_detect_enqueue") and hasattr(lib, "agx_group_detect_fetch")
    from aprilgrid_rs_amd import DetectorGroup
    for name in ("detect_enqueue", "detect_fetch", "detect_fetch_raw"):
        assert callable(getattr(DetectorGroup, name))


def test_a_null_group_is_an_argument_error_without_hip():
    lib = _lib()
    frames = (C.c_void_p * 1)(None)
    assert lib.agx_group_detect_enqueue(None, frames, 4, 640, 400, 640, 640 * 400, 0, 1024, 0) == AGX_ERR_ARG
    assert lib.agx_group_detect_enqueue(None, None, 4, 640, 400, 640, 640 * 400, 0, 1024, 0) == AGX_ERR_ARG
    counts = (C.c_uint32 * 4)()
    out = (C.c_uint8 * (4 * 36))()
    assert lib.agx_group_detect_fetch(None, out, counts, None, 0) == AGX_ERR_ARG
    assert lib.agx_group_detect_fetch(None, None, None, None, 0) == AGX_ERR_ARG
    assert b"null" in lib.agx_group_last_error(None)
