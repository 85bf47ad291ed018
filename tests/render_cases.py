"""Cases and a numpy float64 restatement for the board renderer (agx_render_boards_enqueue / _tail): shared by
tests/test_render_cpu.py and tests/test_gpu_render.py.

The restatement shares nothing with csrc/render_math.h but the definition of the picture: its forward models are the ones the pose
tests restate (tests/board_pose_ds_cases.py: project, all three lens models), its inverse is its own -- the nearest point of a
dense grid of projected board points as the seed, then Newton steps with a central-difference Jacobian -- and the board is drawn
from the printed layout's description (a black square at every lattice point, tags with border and code bits, rows from the top).
"""
import numpy as np

import aprilgrid_rs_amd as A
from aprilgrid_rs_amd import _ffi, synth
from tests import board_pose_cases as PC
from tests import board_pose_ds_cases as DC

SMALL = (96, 80)  # w, h of the restated frames
# cameras for SMALL frames: one per lens model, and a double-sphere lens so short that a near, tilted board passes 90 degrees
SMALL_CAMERAS = {
    "radtan": A.Camera(70.0, 72.0, 47.3, 40.2, -0.12, 0.03, 0.002, -0.001, 0.004),
    "equi": A.Camera.equidistant(45.0, 46.0, 48.4, 39.1, -0.013, 0.021, -0.013, 0.0026),
    "ds": A.Camera.double_sphere(62.0, 61.0, 47.6, 40.3, 0.6, 0.45),
    "ds_past_90": A.Camera.double_sphere(24.0, 24.0, 48.2, 39.7, -0.2, 0.59),
}
# (distance, tilt_x, tilt_y, roll, offset) per camera and layout, board_pose_looking_at's arguments, tag_size 1
SMALL_POSES = {
    ("radtan", (2, 3)): (5.1, 17.0, -23.0, 31.0, (0.21, -0.13)),
    ("radtan", (1, 1)): (2.3, -21.0, 14.0, -37.0, (-0.11, 0.07)),
    ("equi", (2, 3)): (3.4, 23.0, 19.0, -52.0, (0.17, 0.12)),
    ("equi", (1, 1)): (1.6, 12.0, -27.0, 64.0, (0.05, -0.09)),
    ("ds", (2, 3)): (4.3, -19.0, 26.0, 73.0, (-0.23, 0.15)),
    ("ds", (1, 1)): (2.1, 28.0, 11.0, -16.0, (0.08, 0.11)),
    ("ds_past_90", (2, 3)): (0.45, 9.0, 48.0, 22.0, (1.35, 0.1)),
    ("ds_past_90", (1, 1)): (0.2, -7.0, 55.0, -13.0, (0.75, -0.05)),
}
# the round trip: 640 x 480, a 6 x 6 board, field angles moderate enough that the oracle's detect finds all 36
TRIP_SIZE = (640, 480)
TRIP_CAMERAS = {
    "radtan": A.Camera(470.0, 474.0, 322.0, 238.0, -0.18, 0.06, 0.001, -0.0015, 0.0),
    "equi": A.Camera.equidistant(430.0, 432.0, 318.0, 243.0, -0.013, 0.021, -0.013, 0.0026),
    "ds": A.Camera.double_sphere(640.0, 644.0, 321.0, 239.0, 0.6, 0.45),
}
TRIP_POSE = (12.0, 14.0, -17.0, 21.0, (0.3, -0.2))


def looking_at(spec):
    d, tx, ty, rz, off = spec
    return A.board_pose_looking_at(d, tx, ty, rz, off)


def colours(dtype):
    """black, white, background of the restated frames: distinct, and white - black no multiple of 16"""
    return (23, 231, 117) if np.dtype(dtype) == np.uint8 else (2111, 60013, 30011)


def _invert(cam, R, t, u, v, half_w, half_h):
    """Board points (X, Y) whose projection is (u, v) [n], and whether one was found within 1e-6 px."""
    from scipy.spatial import cKDTree
    gx, gy = np.meshgrid(np.linspace(-half_w, half_w, 161), np.linspace(-half_h, half_h, 161))
    G = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], axis=-1)
    uvg = DC.project(cam, R, t, G)
    ok = np.isfinite(uvg).all(axis=1)
    G, uvg = G[ok], uvg[ok]
    if not len(G):
        return np.zeros_like(u), np.zeros_like(v), np.zeros(u.shape, bool)
    _, near = cKDTree(uvg).query(np.stack([u, v], axis=-1))
    X, Y = G[near, 0].copy(), G[near, 1].copy()

    def f(X, Y):
        return DC.project(cam, R, t, np.stack([X, Y, np.zeros_like(X)], axis=-1))

    h = 1e-6
    with np.errstate(invalid="ignore", divide="ignore"):
        for _ in range(12):
            p = f(X, Y)
            jx, jy = (f(X + h, Y) - f(X - h, Y)) / (2 * h), (f(X, Y + h) - f(X, Y - h)) / (2 * h)
            e0, e1 = u - p[:, 0], v - p[:, 1]
            det = jx[:, 0] * jy[:, 1] - jy[:, 0] * jx[:, 1]
            dX, dY = (jy[:, 1] * e0 - jy[:, 0] * e1) / det, (jx[:, 0] * e1 - jx[:, 1] * e0) / det
            good = np.isfinite(dX) & np.isfinite(dY)
            X, Y = np.where(good, X + dX, X), np.where(good, Y + dY, Y)
        p = f(X, Y)
        found = np.hypot(u - p[:, 0], v - p[:, 1]) < 1e-6
    return X, Y, found


def restated(size, cols, rows, cam, R, t, family="T36H11", first_id=0, s=0.3, tag_size=1.0, margin=0.5, S=2, dtype=np.uint8,
             colours_=None):
    """-> (frame [h, w], the smallest distance of an on-page sample to an edge of the drawing in tag sides, the number of accepted
    samples whose camera-frame Z is <= 0)."""
    w, h = size
    black, white, bg = colours_ or colours(dtype)
    codes = synth.family_codes(family)
    _, edge, border = synth.FAMILY_LAYOUT[family]
    n = edge + 2 * border
    pitch = 1.0 + s
    ws, hs = cols * pitch + s, rows * pitch + s
    off = (np.arange(S) + 0.5) / S - 0.5
    uu = (np.arange(w)[None, :, None, None] + off[None, None, None, :]) + np.zeros((h, 1, S, 1))
    vv = (np.arange(h)[:, None, None, None] + off[None, None, :, None]) + np.zeros((1, w, 1, S))
    u, v = uu.ravel(), vv.ravel()
    X, Y, found = _invert(cam, R, t, u, v, (ws / 2 + margin) * tag_size, (hs / 2 + margin) * tag_size)
    xs, ys = X / tag_size + ws / 2, Y / tag_size + hs / 2
    on_page = found & (xs >= -margin) & (xs <= ws + margin) & (ys >= -margin) & (ys <= hs + margin)
    in_board = (xs >= 0) & (xs < ws) & (ys >= 0) & (ys < hs)
    i, j = np.floor(xs / pitch), np.floor(ys / pitch)
    fx, fy = xs - i * pitch, ys - j * pitch
    square = in_board & (fx < s) & (fy < s)
    tag = in_board & (fx >= s) & (fy >= s) & (i < cols) & (j < rows)
    cx = np.clip(np.floor((fx - s) * n), 0, n - 1).astype(int)
    cy = np.clip(np.floor((fy - s) * n), 0, n - 1).astype(int)
    row, col = n - 1 - cy - border, cx - border  # the tag's rows are printed from its top: Y's high end
    inner = (row >= 0) & (row < edge) & (col >= 0) & (col < edge)
    tid = (np.clip(j, 0, rows - 1) * cols + np.clip(i, 0, cols - 1)).astype(int)
    code = np.array([codes[first_id + k] for k in range(rows * cols)], dtype=np.uint64)[tid]
    shift = (edge * edge - 1 - (np.clip(row, 0, edge - 1) * edge + np.clip(col, 0, edge - 1))).astype(np.uint64)
    bit = ((code >> shift) & np.uint64(1)) == 1
    is_black = on_page & (square | (tag & ~(inner & bit)))
    is_white = on_page & ~is_black
    ss = S * S
    n_w = is_white.reshape(h, w, ss).sum(axis=2).astype(np.int64)
    n_b = is_black.reshape(h, w, ss).sum(axis=2).astype(np.int64)
    frame = (n_w * white + n_b * black + (ss - n_w - n_b) * bg + ss // 2) // ss
    # distances to the edges of the drawing (page, board, lattice, cells), for the samples on the page
    d = [np.abs(xs + margin), np.abs(xs - ws - margin), np.abs(ys + margin), np.abs(ys - hs - margin), np.abs(xs), np.abs(xs - ws), np.abs(ys),
         np.abs(ys - hs)]
    for q in (fx, fy):
        d += [np.minimum(q, pitch - q), np.abs(q - s)]
        cell = (q - s) * n
        d.append(np.where(q >= s, np.abs(cell - np.round(cell)) / n, np.inf))
    edge_dist = np.min(np.stack(d), axis=0)[on_page].min() if on_page.any() else np.inf
    Zc = X * R[2, 0] + Y * R[2, 1] + t[2]
    return frame.astype(dtype), float(edge_dist), int((on_page & (Zc <= 0.0)).sum())
