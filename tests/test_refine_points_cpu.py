"""rochade_refine of caller-given points (agx_refine_points_enqueue / _fetch, agx_rochade_refine; reference
src/detector.rs:194-361) as far as it can be checked without a device: the header declares the entry points and the enums,
the built library exports them, the ctypes table and ffi.rs bind them, `agx_point` has one layout everywhere, and the gfx950
code object holds k_refine_points without scratch.  Only the code object's metadata is read."""
import ctypes as C
import os
import re
import subprocess
import tempfile

from tests.util import ROOT

HDR = os.path.join(ROOT, "include", "aprilgrid_amd.h")
ENTRY_POINTS = ("agx_refine_points_enqueue", "agx_refine_points_fetch", "agx_rochade_refine")
CONSTANTS = {"AGX_POINT_REFINED": 0, "AGX_POINT_OUTSIDE": 1, "AGX_POINT_NOT_SADDLE": 2, "AGX_POINT_MOVED": 3,
             "AGX_REFINE_BLURRED": 0, "AGX_REFINE_PLANE": 1}


def header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def test_header_declares_the_entry_points_and_the_enums():
    h = header()
    protos = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"^int (agx_\w+)\s*\(([^;]*?)\)\s*;", h, flags=re.M | re.S)}
    for name in ENTRY_POINTS:
        assert name in protos, name
    enq = [a.strip() for a in protos["agx_refine_points_enqueue"].split(",")]
    assert [a.split()[-1].lstrip("*") for a in enq] == ["det", "d_frames", "n_frames", "width", "height", "row_stride_bytes",
                                                        "frame_stride_bytes", "format", "image", "d_points", "points_per_frame",
                                                        "d_counts", "d_out", "d_status"]
    assert "half_size_patch" not in " ".join(protos[n] for n in ENTRY_POINTS)  # it is 2: there is no parameter for it
    assert [a.strip().split()[-1].lstrip("*") for a in protos["agx_refine_points_fetch"].split(",")] == ["det", "out", "status"]
    assert [a.strip().split()[-1].lstrip("*") for a in protos["agx_rochade_refine"].split(",")] == [
        "det", "pixels", "width", "height", "row_stride_bytes", "format", "image", "points", "n_points", "out", "status", "n_refined"]
    in_header = {n: int(v) for body in re.findall(r"enum\s*\w*\s*\{(.*?)\}", h, flags=re.S) for n, v in re.findall(r"\b(AGX_\w+)\s*=\s*(-?\d+)", body)}
    for name, value in CONSTANTS.items():
        assert in_header.get(name) == value, name
    # every new declaration names the reference's lines
    raw = open(HDR).read()
    for name in ENTRY_POINTS:
        at = raw.index("int " + name)
        assert "src/detector.rs:194-361" in raw[raw.rindex("/*", 0, at):at], name


def test_library_exports_and_ctypes_table_binds_them():
    from aprilgrid_rs_amd import _ffi
    lib = _ffi.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in ENTRY_POINTS:
        assert re.search(r"\bT %s\b" % name, nm), name
        assert name in _ffi.SYMBOLS and getattr(lib, name).argtypes == _ffi.SYMBOLS[name][1]
    assert len(_ffi.SYMBOLS["agx_refine_points_enqueue"][1]) == 14 and len(_ffi.SYMBOLS["agx_refine_points_fetch"][1]) == 3
    assert len(_ffi.SYMBOLS["agx_rochade_refine"][1]) == 12
    for name, value in CONSTANTS.items():
        assert getattr(_ffi, name) == value, name
    # a NULL handle is an argument error, not a crash (no device is needed for that)
    assert lib.agx_refine_points_fetch(None, None, None) == _ffi.AGX_ERR_ARG
    assert lib.agx_refine_points_enqueue(None, None, 1, 16, 16, 16, 256, 0, 0, None, 1, None, None, None) == _ffi.AGX_ERR_ARG
    assert lib.agx_rochade_refine(None, None, 16, 16, 16, 0, 0, None, 0, None, None, None) == _ffi.AGX_ERR_ARG


def test_agx_point_has_one_layout_in_the_header_ctypes_numpy_and_rust():
    """struct agx_point { float x, y; }: 8 bytes, x first -- the header, _ffi.PointC, _ffi.POINT_DTYPE and ffi.rs's #[repr(C)] struct."""
    import numpy as np
    from aprilgrid_rs_amd import _ffi
    m = re.search(r"struct agx_point\s*\{(.*?)\}\s*;", header(), flags=re.S)
    assert m and " ".join(m.group(1).split()) == "float x, y;"
    assert re.search(r"typedef struct agx_point agx_point;", header())
    assert C.sizeof(_ffi.PointC) == 8 and [f[0] for f in _ffi.PointC._fields_] == ["x", "y"]
    assert all(f[1] is C.c_float for f in _ffi.PointC._fields_)
    dt = np.dtype(_ffi.POINT_DTYPE)
    assert dt.itemsize == 8 and dt.names == ("x", "y") and dt["x"] == np.float32 and dt.fields["y"][1] == 4
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read())
    r = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^\]]*\)\]\s*)?pub\s+struct\s+agx_point\s*\{(.*?)\}", rust, flags=re.S)
    assert r and [" ".join(f.split()) for f in r.group(1).split(",") if f.strip()] == ["pub x: c_float", "pub y: c_float"]
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert re.search(r"pub fn rochade_refine\(&self, img: &image::DynamicImage, initial_corners: &\[\(f32, f32\)\]\) -> Vec<Saddle>", lib_rs)
    assert re.search(r"pub fn rochade_refine_with_status\(", lib_rs)


def test_compiled_refine_points_kernel_uses_no_scratch_and_no_lds():
    """The gfx950 code object inside the built library (metadata notes only): both instantiations of k_refine_points -- the
    aligned 16-byte window loads for the chain's blur plane, single floats for a caller's plane -- are there, with no private
    segment (no scratch, no register spilled to memory) and no LDS; one wave per workgroup."""
    llvm = "/opt/rocm/lib/llvm/bin"
    lib = os.path.join(ROOT, "aprilgrid-rs_amd", "libaprilgrid_amd.so")
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
        subprocess.run([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "unused")],
                       check=True, capture_output=True)
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True, capture_output=True)
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    kernels = {}
    for blk in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "k_refine_points" in name:
            kernels[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                             for k in ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count", "vgpr_spill_count",
                                       "max_flat_workgroup_size")}
    assert len(kernels) == 2, sorted(kernels)
    assert not any("k_front_luma" in name for name in kernels)  # (tests/test_formats_cpu.py counts kernels by that name)
    for name, k in kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_count"] <= 128, (name, k)  # (at least four waves per SIMD)
        assert k["max_flat_workgroup_size"] == 64, (name, k)
