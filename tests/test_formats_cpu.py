"""The integer layouts behind the front-end kernel (AGX_LA8 .. AGX_RGBA16), as far as they can be checked without a device:
the host's to_luma8 (agx_luma8) of every one of them against a numpy restatement of the header's table, byte for byte on
every pixel, the agreement of the header, _ffi.py and ffi.rs on the eight constants, and the resources of the compiled kernel.

The kernel and the host divide by 10000 with a plain `/`: there is no hand-written multiply-shift whose exactness would have
to be checked over the numerators (the compiler's own sequence for a division by a constant is exact by construction)."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, PAD = 97, 61, 5  # an odd width, rows PAD pixels longer than the image

FORMATS = {"AGX_LA8": 4, "AGX_RGBA8": 5, "AGX_BGR8": 6, "AGX_BGRA8": 7, "AGX_RGB8P": 8, "AGX_LA16": 9, "AGX_RGB16": 10,
           "AGX_RGBA16": 11}


@pytest.fixture(scope="module")
def lib():
    from aprilgrid_rs_amd import _ffi
    return _ffi.lib()


def weighted(r, g, b):
    """(2126 R + 7152 G + 722 B) / 10000 in unsigned 32-bit arithmetic (at most 655 350 000 for 16-bit channels)."""
    n = 2126 * r.astype(np.uint64) + 7152 * g.astype(np.uint64) + 722 * b.astype(np.uint64)
    assert int(n.max()) < 2 ** 32
    return (n // 10000).astype(np.uint32)


def build_layout(name, rng, w=W, h=H, pad=PAD):
    """-> (array as the library is handed it, with rows `pad` pixels longer than w filled with other bytes; row stride in
    bytes; expected to_luma8 [h, w]; the underlying RGB8 image or None)."""
    wide = w + pad
    if name in ("AGX_LA16", "AGX_RGB16", "AGX_RGBA16"):
        ch = {"AGX_LA16": 2, "AGX_RGB16": 3, "AGX_RGBA16": 4}[name]
        px = rng.integers(0, 65536, (h, wide, ch), dtype=np.uint16)
        px[0, 0] = 65535  # the largest numerator
        px[0, 1] = 0
        v = px[:, :w].astype(np.uint32)
        l16 = v[..., 0] if name == "AGX_LA16" else weighted(v[..., 0], v[..., 1], v[..., 2])
        return px, wide * ch * 2, ((l16 + 128) // 257).astype(np.uint8), None
    rgb = rng.integers(0, 256, (h, wide, 3), dtype=np.uint8)
    rgb[0, 0] = 255
    rgb[0, 1] = 0
    alpha = rng.integers(0, 256, (h, wide, 1), dtype=np.uint8)
    want = weighted(rgb[:, :w, 0], rgb[:, :w, 1], rgb[:, :w, 2]).astype(np.uint8)
    base = np.ascontiguousarray(rgb[:, :w])
    if name == "AGX_LA8":
        return np.concatenate([rgb[..., :1], alpha], -1), wide * 2, rgb[:, :w, 0].copy(), None
    if name == "AGX_RGBA8":
        return np.concatenate([rgb, alpha], -1), wide * 4, want, base
    if name == "AGX_BGR8":
        return np.ascontiguousarray(rgb[..., ::-1]), wide * 3, want, base
    if name == "AGX_BGRA8":
        return np.concatenate([rgb[..., ::-1], alpha], -1), wide * 4, want, base
    if name == "AGX_RGB8P":
        return np.ascontiguousarray(rgb.transpose(2, 0, 1)), wide, want, base
    raise ValueError(name)


@pytest.mark.parametrize("name", sorted(FORMATS))
def test_host_luma8_of_every_new_layout(lib, name):
    """agx_luma8 on a 97 x 61 image with a padded row stride == the numpy restatement, every pixel; for the layouts derived
    from an RGB8 image also the oracle's to_luma8 of that image."""
    rng = np.random.default_rng(FORMATS[name])
    px, stride, want, base = build_layout(name, rng)
    px = np.ascontiguousarray(px)
    out = np.full((H, W), 0xEE, np.uint8)
    assert lib.agx_luma8(px.ctypes.data, W, H, stride, FORMATS[name], out.ctypes.data) == 0
    assert out.tobytes() == want.tobytes(), np.argwhere(out != want)[:5]
    if base is not None:
        from oracle import oracle as O
        assert np.array_equal(out, O.luma_u8(base))


def test_host_luma8_still_refuses_what_it_refused(lib):
    px = np.zeros((4, 4), np.float32)
    out = np.zeros((4, 4), np.uint8)
    assert lib.agx_luma8(px.ctypes.data, 4, 4, 16, 3, out.ctypes.data) == -2   # AGX_LF32
    assert lib.agx_luma8(px.ctypes.data, 4, 4, 16, 12, out.ctypes.data) == -2  # no such format
    assert lib.agx_luma8(px.ctypes.data, 4, 4, 16, -1, out.ctypes.data) == -2
    assert lib.agx_abi_version() == 1


def test_python_wrapper_infers_and_overrides_formats():
    import aprilgrid_rs_amd as A
    from aprilgrid_rs_amd import _ffi
    rng = np.random.default_rng(5)
    for name in sorted(FORMATS):
        px, _, _, _ = build_layout(name, rng, pad=0)
        got = A.TagDetector.luma8(px, format=FORMATS[name])
        out = np.zeros((H, W), np.uint8)
        px = np.ascontiguousarray(px)
        row = px.strides[-2] if name == "AGX_RGB8P" else px.strides[0]
        assert _ffi.lib().agx_luma8(px.ctypes.data, W, H, row, FORMATS[name], out.ctypes.data) == 0
        assert np.array_equal(got, out), name
        if name not in ("AGX_BGR8", "AGX_BGRA8", "AGX_RGB8P"):  # these can only be named
            assert np.array_equal(A.TagDetector.luma8(px), out), name
    with pytest.raises(A.AgxError) as e:
        A.TagDetector.luma8(np.zeros((8, 8, 3), np.uint8), format=_ffi.AGX_RGBA8)
    assert e.value.status == _ffi.AGX_ERR_FORMAT
    with pytest.raises(A.AgxError) as e:
        A.TagDetector.luma8(np.zeros((8, 8), np.uint8), format=12)
    assert e.value.status == _ffi.AGX_ERR_FORMAT


def test_header_ffi_py_and_ffi_rs_agree_on_the_constants():
    from aprilgrid_rs_amd import _ffi
    header = open(os.path.join(ROOT, "include", "aprilgrid_amd.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    body = re.search(r"typedef enum agx_format \{(.*?)\} agx_format;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    in_header = {m.group(1): int(m.group(2)) for m in re.finditer(r"(AGX_\w+)\s*=\s*(\d+)", body)}
    in_rust = {m.group(1): int(m.group(2)) for m in re.finditer(r"pub const (AGX_\w+): c_int = (\d+);", rust)}
    assert in_header == dict(FORMATS, AGX_L8=0, AGX_L16=1, AGX_RGB8=2, AGX_LF32=3)
    for name, value in FORMATS.items():
        assert in_rust.get(name) == value, name
        assert getattr(_ffi, name) == value, name
        assert value in _ffi.FORMAT_LAYOUT
    assert re.search(r"#define AGX_ABI_VERSION 1\b", header)


def test_compiled_front_kernel_uses_no_scratch_and_loads_vectors():
    """The gfx950 code object inside the built library: every k_front_luma instantiation (8 layouts + the 3 narrowing ones of the
    16-bit layouts) has no scratch and no LDS, and its vector path loads dword vectors (dwordx2 / x3 / x4 as the layout needs)
    and stores one dword (u8 planes) or two (u16 planes)."""
    llvm = "/opt/rocm/lib/llvm/bin"
    lib = os.path.join(ROOT, "aprilgrid-rs_amd", "libaprilgrid_amd.so")
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
        subprocess.run([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "unused")],
                       check=True, capture_output=True)
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True, capture_output=True)
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        text = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
    kernels = {}
    for blk in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "k_front_luma" in name:
            kernels[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                             for k in ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count")}
    assert len(kernels) == 11, sorted(kernels)
    for name, k in kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_count"] <= 64, (name, k)  # (8 waves per SIMD)
    bodies = {}
    cur = None
    for line in text.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\w+)>:", line)
        if m:
            cur = m.group(1)
            bodies[cur] = []
        elif cur:
            bodies[cur].append(line)
    want_load = {4: "global_load_dwordx2", 5: "global_load_dwordx4", 6: "global_load_dwordx3", 7: "global_load_dwordx4",
                 8: "global_load_dword ", 9: "global_load_dwordx4", 10: "global_load_dwordx4", 11: "global_load_dwordx4"}
    for name in kernels:
        layout, out8 = re.search(r"k_front_lumaILi(\d+)ELb([01])E", name).groups()
        body = "\n".join(bodies[name])
        assert want_load[int(layout)] in body, name
        assert ("global_store_dwordx2" if int(layout) >= 9 and out8 == "0" else "global_store_dword ") in body, name
        assert "scratch_" not in body and "ds_" not in body, name
