"""The yardstick of the chain at any half_size_patch: TagDetector::refined_saddle_points (src/detector.rs:408-446) with the
`1.5` of :410 replaced by a sigma and the `2` of :430 by a half_size_patch, composed from the oracle's exported pieces exactly
as tests/sigma_oracle.py is -- the one difference is the third argument of orc_rochade_refine.  tests/test_patch_cpu.py holds
the composition at (1.5, 2) to O.refined_saddle_points(img, debug=True), product by product and bit for bit;
tests/test_gpu_patch.py compares the detector with it at the other sizes."""
import numpy as np

from oracle import oracle as O


def refined_saddle_points(img, sigma, half, params=None):
    """-> (saddles after the k / phi filter, dict of the intermediate products with the keys of O.refined_saddle_points'
    debug dict: blur, resp, min_resp, centers, first_index, sizes, refined)."""
    lib = O.lib()
    prm = params or O.default_params()
    blur = O.gaussian_blur_f32(O.luma_f32(img), float(np.float32(sigma)))  # :409-410
    h, w = blur.shape
    resp = O.hessian_response(blur)  # :411
    min_resp = np.float32(lib.orc_min_response(resp.ctypes.data, resp.size))  # :414-417
    thr = np.float32(min_resp * np.float32(0.05))  # :418
    cap = resp.size // 2 + 16
    centers = np.zeros((cap, 2), np.float32)
    first_index = np.zeros(cap, np.uint32)
    sizes = np.zeros(cap, np.uint32)
    work = resp.copy()  # (pixel_bfs overwrites what it visits)
    nc = lib.orc_cluster_centers(work.ctypes.data, w, h, thr, centers.ctypes.data, first_index.ctypes.data, sizes.ctypes.data, cap)
    assert 0 <= nc <= cap
    centers, first_index, sizes = centers[:nc].copy(), first_index[:nc].copy(), sizes[:nc].copy()
    refined = np.zeros(max(nc, 1), O.SADDLE_DTYPE)
    nr = lib.orc_rochade_refine(blur.ctypes.data, w, h, centers.ctypes.data, nc, int(half), refined.ctypes.data)  # :430
    refined = refined[:nr].copy()
    out = refined
    if nr:  # :431-445, in f32
        s_max_k = np.float32(refined["k"].max() / np.float32(10))
        keep = (refined["k"] >= s_max_k) & (refined["phi"] >= np.float32(prm.min_saddle_angle)) & (refined["phi"] <= np.float32(prm.max_saddle_angle))
        out = refined[keep].copy()
    d = dict(blur=blur, resp=resp, min_resp=min_resp, centers=centers, first_index=first_index, sizes=sizes, refined=refined)
    return out, d
