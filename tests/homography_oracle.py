"""The yardstick of the homography sampling model: reference src/image_util.rs:5-37 (tag_homography) restated in numpy float64 --
the 8 x 9 matrix of the four correspondences and the last right-singular vector of its SVD -- plus what the tests build on it:
the sample points, the inverse map, quads of a given perspective and hand-painted perspective tags.  Numpy only.

No reference binary can be built here (__graft_entry__.py: the reference is a Rust crate with un-vendored dependencies), so the
restatement is the yardstick.  The reference's vector has unit norm and the sign its SVD happens to give; a consumer divides by
w, so maps are compared projectively: through the points they give, after scaling w at the source square's centre to 1."""
import numpy as np

from tests import tag_cases as T

DEGENERATE = 6  # AGX_QUAD_DEGENERATE
SKIPPED = 5


def source_square(side_bits, margin):
    """tag_affine's / tag_homography's source corners (-m, -m), (-m, S), (S, S), (S, -m), S = (float)side_bits - 1 + margin"""
    m = float(np.float32(margin))
    s = float(np.float32(np.float32(side_bits) - np.float32(1.0) + np.float32(margin)))
    return np.array([[-m, -m], [-m, s], [s, s], [s, -m]], np.float64)


def dlt(src, dst):
    """image_util.rs:15-31: two rows per correspondence, the SVD's last right-singular vector as a 3 x 3 matrix"""
    a = np.zeros((8, 9), np.float64)
    for i, ((x, y), (u, v)) in enumerate(zip(np.asarray(src, np.float64), np.asarray(dst, np.float64))):
        a[2 * i] = [-x, -y, -1, 0, 0, 0, x * u, y * u, u]
        a[2 * i + 1] = [0, 0, 0, -x, -y, -1, x * v, y * v, v]
    return np.linalg.svd(a)[2][-1].reshape(3, 3)


def tag_homography(quad, side_bits, margin):
    """The reference's map of the source square onto the quad (float64), scaled to w = 1 at the square's centre"""
    src = source_square(side_bits, margin)
    h = dlt(src, np.asarray(quad, np.float64).reshape(4, 2))
    c = src.mean(axis=0)
    return h / (h[2, 0] * c[0] + h[2, 1] * c[1] + h[2, 2])


def apply(h, xy):
    """The images of the points xy [n, 2] under the 3 x 3 map -> [n, 2] float64"""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    p = np.concatenate([xy, np.ones((len(xy), 1))], axis=1) @ np.asarray(h, np.float64).T
    return p[:, :2] / p[:, 2:3]


def grid(border, edge):
    """decode_positions' source coordinates (:60-70): x outer, y inner -> [edge^2, 2]"""
    g = np.arange(border, border + edge, dtype=np.float64)
    return np.stack([np.repeat(g, edge), np.tile(g, edge)], axis=1)


def positions(quad, border, edge, margin):
    """The exact homography's sample points of the quad -> [edge^2, 2] float64"""
    return apply(tag_homography(quad, 2 * border + edge, margin), grid(border, edge))


def trapezoid(cx, cy, side, ratio, turn=0.0, lean=0.0):
    """A convex quad: near edge `side` px, far edge ratio * side px, `side` px apart, the far edge pushed sideways by lean * side,
    turned by `turn` radians about (cx, cy) -> [4, 2] float32, corners in the order of the source square's"""
    far = 0.5 * ratio * side
    q = np.array([[-far + lean * side, -0.5 * side], [far + lean * side, -0.5 * side], [0.5 * side, 0.5 * side], [-0.5 * side, 0.5 * side]])
    c, s = np.cos(turn), np.sin(turn)
    return (q @ np.array([[c, s], [-s, c]]) + [cx, cy]).astype(np.float32)


# ---- hand-painted perspective tags --------------------------------------------------------------------------------------------
PAINT_W, PAINT_H = T.TAIL_SIZE
PAINT_RATIO = 0.6     # far edge / near edge of the painted tag's trapezoid
PAINT_SIDE = 320      # px, the near edge
PAINT_CODE = {"T16H5": 7, "T25H7": 11, "T25H9": 5, "T36H11": 23, "T36H11B1": 23}


def painted_quad():
    """The painted tags' quad: corner 0 -> corner 1 is the far edge (source y runs along it)"""
    return trapezoid(400.0, 300.0, PAINT_SIDE, PAINT_RATIO)


def paint_perspective(fam, quad, code, margin=0.5, lo=20, hi=235, ground=128):
    """An 800 x 600 L8 plane with the family's tag `code` under `quad`: every pixel centre is mapped back through the yardstick's
    inverse map to source coordinates; a pixel inside the source square takes its cell's value (cell of source (x, y): x, y rounded;
    border cells dark, data cell n = (x - border) * edge + (y - border) bright where the code has bit nb - 1 - n), else `ground`.
    -> (plane, cells [H, W] int: the sample number of a data cell's pixels, -1 elsewhere)"""
    edge, border, _, codes = T.family(fam)
    side = edge + 2 * border
    nb = edge * edge
    hinv = np.linalg.inv(tag_homography(quad, side, margin))
    ys, xs = np.mgrid[0:PAINT_H, 0:PAINT_W]
    s = apply(hinv, np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float64))
    m = float(margin)
    inside = ((s > -m) & (s < side - 1 + m)).all(axis=1)
    cx, cy = np.floor(s[:, 0] + 0.5).astype(np.int64), np.floor(s[:, 1] + 0.5).astype(np.int64)
    data = inside & (cx >= border) & (cx < border + edge) & (cy >= border) & (cy < border + edge)
    n = np.where(data, (cx - border) * edge + (cy - border), -1)
    word = int(codes[code])
    bit = np.array([(word >> (nb - 1 - k)) & 1 for k in range(nb)] + [0], np.int64)  # (index -1: the frame, dark)
    plane = np.where(inside, np.where(bit[n] == 1, hi, lo), ground).astype(np.uint8)
    return plane.reshape(PAINT_H, PAINT_W), n.reshape(PAINT_H, PAINT_W)


def painted_case(fam):
    """-> (plane, cells, quad [4, 2] float32, code index) of the family's painted perspective tag"""
    quad = painted_quad()
    code = PAINT_CODE[fam]
    plane, cells = paint_perspective(fam, quad, code)
    return plane, cells, quad, code
