"""Hand-built saddle lists for the board search (agx_find_board_tail, k_find_boards): exact lattices, lists in another index
order, coincident saddles, saddles exactly on a 3-NN query's radius, lattices at the values of a parameter where the search's
answer changes, and lists around the kernel's fixed sizes.  Numpy only; what every case claims is asserted from the oracle and
numpy in tests/test_board_cases_cpu.py, and tests/test_gpu_board_lattices.py runs the lists through the kernel.

A list is [n, 5] float32: x, y, k, theta, phi (k = phi = 0: the search never reads them).  The basic lattice has the spacing 20,
its saddle of row r and column c at list position r * cols + c, and theta +45 / -45 by the parity of r + c: every other cell of
it is a valid quad (7 x 7 saddles show 9 quads, 13 x 13 show 36: the `quads` a case claims are the oracle's counts).

A case's `expect`:
  "device"      the kernel must answer it (no AGX_BOARD_PENDING before the fetch);
  "limit-pair"  one of a straddling pair (PAIRS): the small one is answered by the kernel, the large one is handed back;
  "any"         either; the answer after the fetch is the host form's in every case."""
import collections

import numpy as np

Case = collections.namedtuple("Case", "name family expect build quads")  # quads: the claimed count (None: no board; -1: no claim)
F32 = np.float32


def f32_steps(v, k):
    """The float32 k steps above (k < 0: below) v."""
    v = F32(v)
    i = np.array([v]).view(np.int32)[0]
    i = i if i >= 0 else np.int32(-2147483648) - i  # a monotone integer line through -0.0 / +0.0
    i = np.int64(i) + k
    i = i if i >= 0 else -2147483648 - i
    return np.array([i], np.int64).astype(np.int32).view(np.float32)[0]


def wrap180(t):
    t = np.asarray(t, np.float64)
    return np.where(t > 180.0, t - 360.0, np.where(t < -180.0, t + 360.0, t))


def lattice(rows, cols, spacing=20.0, origin=(100.0, 60.0), rot=0.0, thetas=(45.0, -45.0), dtheta=F32(0.0), shear=F32(0.0), homography=None):
    """rows x cols saddles, row-major.  Coordinates in float64 -- x = (c + shear * r) * spacing, y = r * spacing, an optional
    projective map of that, rotated by `rot` degrees about (0, 0), moved to `origin` -- and rounded once to float32.  theta =
    float32(thetas[parity] + dtheta), in float32, plus rot (thetas are directions in the same coordinates: they turn along)."""
    r, c = np.mgrid[0:rows, 0:cols]
    x = (c + float(F32(shear)) * r) * float(spacing)
    y = r * float(spacing)
    if homography is not None:
        g, h = homography
        w = 1.0 + g * x + h * y
        x, y = x / w, y / w
    a = np.deg2rad(float(rot))
    xr, yr = x * np.cos(a) - y * np.sin(a), x * np.sin(a) + y * np.cos(a)
    out = np.zeros((rows * cols, 5), F32)
    out[:, 0] = (xr + origin[0]).ravel()
    out[:, 1] = (yr + origin[1]).ravel()
    base = np.where((r + c) % 2 == 0, F32(thetas[0]), F32(thetas[1])).astype(F32) + F32(dtheta)  # float32 arithmetic
    out[:, 3] = wrap180(base.astype(np.float64) + float(rot)).ravel()
    return out


def far_saddles(n, seed, lo=3000.0, hi=9000.0):
    """Sparse saddles far from any lattice here, their thetas spread over 170 bins: none a seed bin of its own weight."""
    rng = np.random.default_rng(seed)
    pad = np.zeros((n, 5), F32)
    pad[:, 0] = rng.uniform(lo, hi, n)
    pad[:, 1] = rng.uniform(lo, hi, n)
    pad[:, 3] = (np.arange(n) % 170 - 85) + 0.25
    return pad


def permuted(l, seed):
    """-> (list, perm): list[i] = l[perm[i]]."""
    perm = np.random.default_rng(seed).permutation(len(l))
    return l[perm].copy(), perm


def repeated(l, k):
    """Every saddle listed k times, the copies next to each other."""
    return np.repeat(l, k, axis=0)


# ---- family 4: a saddle on the radius of a 3-NN query decides the board ------------------------------------------------------
# tail_kernels.hip expand_one_w / board.rs:177-233: for a pair (a, b) of a quad's saddles and the anchor a,
#   radius_sq = 0.5f * (ex * ex + ey * ey), e = a - b;  q = a + (b - a) * (1.0f + 0.3f);  a saddle p of the anchor's orientation
#   counts if dx * dx + dy * dy <= radius_sq with d = q - p.
# A strip of 2 x 5 saddles of spacing 32 (|a - b|^2 = 1024, radius_sq = 512 exactly; (b - a) * 1.3f = 32 * 1.3f exactly, a power
# of two).  Its valid cells are columns 1-2 and 3-4.  The thetas leave the search one seed, saddle (1, 1) -- its bin 45 holds it
# and a far saddle, every other bin one saddle --, so the only board grows from cell 1-2, and cell 3-4 joins it only through the
# query of pair a = (0, 1), b = (0, 2): q = a + (41.6, 0), whose one candidate of a's orientation is saddle (0, 3).  That saddle
# is moved from q + (22.4, 0) to q + (dx, dy) with dx * dx + dy * dy == 512 in float32, bit for bit (RADIUS_DY; dx is searched
# for among the float32 next to sqrt(512 - dy^2)): with `<=` the board has two quads, one float32 step of x further out it has one.
RADIUS_SPACING = 32.0
RADIUS_ORIGIN = (64.0, 64.0)
RADIUS_DY = (2.75, 3.75, 4.0, -2.75, -3.75, -4.0)  # the dy for which an exact dx exists
RADIUS_AT = 3  # list position of the moved saddle (0, 3)
RADIUS_THETAS = {0: 43.0, 6: 45.0, 2: 46.0, 8: 47.0, 4: 48.0, 5: -45.0, 1: -44.0, 7: -43.0, 3: -42.0, 9: -41.0}


def radius_query(l, cols, r, c, dr, dc):
    """The kernel's expressions in float32 for the pair a = (r, c), b = (r + dr, c + dc), anchor a -> (qx, qy, radius_sq)."""
    a, b = l[r * cols + c], l[(r + dr) * cols + c + dc]
    ex, ey = F32(a[0] - b[0]), F32(a[1] - b[1])
    radius_sq = F32(F32(0.5) * F32(F32(ex * ex) + F32(ey * ey)))
    ratio0 = F32(F32(1.0) + F32(0.3))
    v10x, v10y = F32(b[0] - a[0]), F32(b[1] - a[1])
    qx, qy = F32(a[0] + F32(v10x * ratio0)), F32(a[1] + F32(v10y * ratio0))
    return qx, qy, radius_sq


def dist_sq(qx, qy, p):
    """dist_key's d2 in float32: dx * dx + dy * dy, d = q - p."""
    dx, dy = F32(F32(qx) - F32(p[0])), F32(F32(qy) - F32(p[1]))
    return F32(F32(dx * dx) + F32(dy * dy))


def on_radius(dy, steps, same_theta=True):
    """The strip with saddle (0, 3) on the radius of the query (steps = 0), or `steps` float32 steps of its x further from the
    query point (negative: nearer).  -> (list, (qx, qy, radius_sq))."""
    l = lattice(2, 5, spacing=RADIUS_SPACING, origin=RADIUS_ORIGIN)
    for i, t in RADIUS_THETAS.items():
        l[i, 3] = t
    qx, qy, rsq = radius_query(l, 5, 0, 1, 0, 1)
    ey = F32(qy + F32(dy))
    centre = F32(float(qx) + np.sqrt(float(rsq) - dy * dy))
    hits = [f32_steps(centre, k) for k in range(-40, 41) if dist_sq(qx, qy, (f32_steps(centre, k), ey)) == rsq]
    assert hits, dy
    l[RADIUS_AT, 0], l[RADIUS_AT, 1] = f32_steps(hits[0], steps), ey
    if not same_theta:
        l[RADIUS_AT, 3] = 42.0
    far = np.zeros((1, 5), F32)
    far[0, 0] = far[0, 1] = 5000.0
    far[0, 3] = 45.0
    return np.concatenate([l, far]), (qx, qy, rsq)


# ---- family 5: the parameter values where the host form's answer changes ---------------------------------------------------
# Bisected on the CPU with agx_find_board_tail's quad count (bisect_change below), never on the device: the last float32 value
# of the parameter (first element) that still gives the answer of the sweep's low end, the first (second) that does not.  The
# 7 x 7 lattice; `dtheta` is added to both thetas in float32, `shear` moves row r by shear * r * spacing in x.
SWEEPS = {
    # name: (parameter, low end, high end, sign of the lattice's shear / dtheta)
    "dtheta+": ("dtheta", 30.0, 45.0, 1.0),
    "dtheta-": ("dtheta", 30.0, 45.0, -1.0),
    "shear+": ("shear", 0.6, 0.8, 1.0),
    "shear-": ("shear", 0.6, 0.8, -1.0),
}
# filled from bisect_change(name, from_high) (the float32 bits of the lower neighbour; the upper one is the next float32):
# "first" is where the low end's answer stops, "last" where the high end's answer begins -- between the two the search goes
# through further answers.  dtheta 30 is |angle| = 60 of the white-block test (saddle.rs:26-38) for a diagonal at 45 degrees,
# shear 0.732 is tan(60 degrees) - 1.  tests/test_board_cases_cpu.py asserts from the oracle that the two neighbours differ.
THRESHOLDS = {
    ("dtheta+", "first"): 0x41F00002, ("dtheta+", "last"): 0x41F00008,
    ("dtheta-", "first"): 0x41F00000, ("dtheta-", "last"): 0x4205BD5F,
    ("shear+", "first"): 0x3F2FA6E2, ("shear+", "last"): 0x3F3B67B7,
    ("shear-", "first"): 0x3F2C660A, ("shear-", "last"): 0x3F3B67F3,
}
THRESHOLD_STEPS = (0, 1, 10, 100, 10000)


def sweep_list(name, value):
    kind, _, _, sign = SWEEPS[name]
    v = F32(sign) * F32(value)
    return lattice(7, 7, dtheta=v) if kind == "dtheta" else lattice(7, 7, shear=v, origin=(400.0, 60.0))


def bisect_change(name, from_high=False):
    """-> (a float32, its upper neighbour) between which the host form's quads change: the end of the low end's answer, or
    (from_high) the beginning of the high end's."""
    import aprilgrid_rs_amd as A
    _, lo, hi, _ = SWEEPS[name]
    answer = lambda v: A.find_board_tail(sweep_list(name, v), cap=1024)[0].tobytes()
    lo, hi = F32(lo), F32(hi)
    want = answer(hi) if from_high else answer(lo)
    assert answer(lo) != answer(hi)
    while f32_steps(lo, 1) != hi:
        mid = F32((np.float64(lo) + np.float64(hi)) / 2)
        if mid == lo or mid == hi:
            mid = f32_steps(lo, 1)
        if (answer(mid) == want) != from_high:
            lo = mid
        else:
            hi = mid
    return lo, hi


def _bits(u):
    return np.array([u], np.uint32).view(np.float32)[0]


# ---- the table -------------------------------------------------------------------------------------------------------------
# the oracle's quad counts of n x n (and 2 x m) lattices, as tests/test_board_cases_cpu.py finds them
CASES = []
PAIRS = []  # (what, [names answered by the kernel, ascending], [names handed back, ascending]): the innermost two straddle the limit
PERMS = {}  # name of a permuted case -> (name of its base, perm)


def _add(name, family, expect, build, quads=-1):
    assert name not in {c.name for c in CASES}, name
    CASES.append(Case(name, family, expect, build, quads))


def _family1():
    for (r, c, q) in ((2, 2, None), (3, 3, 1), (7, 7, 9), (12, 12, 30), (13, 13, 36), (2, 14, 6)):  # (2 x 30, 20 x 20, 32 x 32: family 6)
        _add("lattice %dx%d" % (r, c), 1, "device", lambda r=r, c=c: lattice(r, c), q)
    _add("lattice 7x7 rows permuted", 1, "device", lambda: lattice(7, 7).reshape(7, 7, 5)[np.random.default_rng(3).permutation(7)].reshape(49, 5), 9)
    _add("lattice 7x7 doubled", 1, "device", lambda: np.concatenate([lattice(7, 7), lattice(7, 7)]), 9)
    _add("lattice 7x7 theta 0/90", 1, "device", lambda: lattice(7, 7, thetas=(0.0, 90.0)), 4)

    def jitter():
        l = lattice(7, 7)
        l[:, :2] += np.random.default_rng(11).normal(0.0, 0.3, (49, 2)).astype(F32)
        return l
    _add("lattice 7x7 jitter 0.3", 1, "device", jitter, 8)  # (the issue's seed gave 7; this one, by the oracle, 8)
    for rot in (0.0, 30.0, 45.0, 90.0):
        _add("lattice 7x7 rot %d" % rot, 1, "device", lambda rot=rot: lattice(7, 7, rot=rot, origin=(300.0, 200.0)), 9)
        _add("lattice 9x9 rot %d" % rot, 1, "device", lambda rot=rot: lattice(9, 9, rot=rot, origin=(300.0, 200.0)), 16)
    for i, hg in enumerate(((2e-4, 1e-4), (-3e-4, 2e-4))):
        _add("lattice 9x9 projective %d" % i, 1, "device", lambda hg=hg, i=i: lattice(9, 9, spacing=30.0, homography=hg, rot=10.0 * i, origin=(300.0, 200.0)))
    for sp in (7.3, 20.1, 33.333):  # x = c * spacing rounds: the products are not exact
        _add("lattice 9x9 spacing %g" % sp, 1, "device", lambda sp=sp: lattice(9, 9, spacing=sp, origin=(0.1, 0.7)), 16)


def _family2():
    for n, q in ((7, 9), (13, 36)):
        base = "lattice %dx%d" % (n, n)
        for seed in range(8):
            name = "%s perm %d" % (base, seed)
            _add(name, 2, "device", lambda n=n, seed=seed: permuted(lattice(n, n), 100 + seed)[0], q)
            PERMS[name] = (base, permuted(lattice(n, n), 100 + seed)[1])
        name = base + " reversed"
        _add(name, 2, "device", lambda n=n: lattice(n, n)[::-1].copy(), q)
        PERMS[name] = (base, np.arange(n * n)[::-1].copy())


def _family3():
    for k in (2, 3):  # (4 times and more: beyond TCAND, family 6)
        _add("7x7 every saddle %d times" % k, 3, "device", lambda k=k: repeated(lattice(7, 7), k), {2: 9, 3: 2}[k])

    def sixty():
        l = lattice(7, 7)
        return np.concatenate([l[:24], np.repeat(l[24:25], 60, axis=0), l[25:]])  # the centre saddle: more than 50 at distance 0
    _add("7x7 centre saddle 60 times", 3, "device", sixty, 9)

    def ulp(k):
        l = lattice(7, 7)
        d = l.copy()
        d[:, 0] = [f32_steps(v, k) for v in d[:, 0]]
        d[:, 1] = [f32_steps(v, -k) for v in d[:, 1]]
        return np.concatenate([l, d])
    _add("7x7 doubled, copies one ulp off", 3, "device", lambda: ulp(1), 9)
    _add("7x7 doubled, copies first, one ulp off", 3, "device", lambda: ulp(1)[::-1].copy(), 9)

    def other_theta(interleaved):
        l = lattice(7, 7)
        d = l.copy()
        d[:, 3] = -d[:, 3]
        return np.stack([l, d], 1).reshape(-1, 5) if interleaved else np.concatenate([d, l])
    _add("7x7 doubled with the other theta", 3, "device", lambda: other_theta(False))
    _add("7x7 doubled with the other theta, interleaved", 3, "device", lambda: other_theta(True))


RADIUS_STEPS = ((0, "on", 2), (-1, "one step inside", 2), (1, "one step outside", 1))  # (steps, what, the quads claimed)


def _family4():
    for dy in RADIUS_DY:
        for steps, what, quads in RADIUS_STEPS:
            _add("radius dy %g: %s" % (dy, what), 4, "device", lambda dy=dy, steps=steps: on_radius(dy, steps)[0], quads)
    _add("radius dy 4: on, other theta", 4, "device", lambda: on_radius(4.0, 0, same_theta=False)[0], 1)  # never a candidate


def threshold_values(name, which):
    """-> [(what, parameter value)]: the two neighbours and 1, 10, 100, 10^4 float32 steps beyond each."""
    lo = _bits(THRESHOLDS[(name, which)])
    hi = f32_steps(lo, 1)
    return [("%d steps below" % k, f32_steps(lo, -k)) for k in THRESHOLD_STEPS] + [("%d steps above" % k, f32_steps(hi, k)) for k in THRESHOLD_STEPS]


def _family5():
    for (name, which) in THRESHOLDS:
        for what, v in threshold_values(name, which):
            # 10^4 float32 steps are 0.02 degrees of dtheta, 6e-4 of shear: two hundred times the kernel's band of 1e-4 degrees
            # around 60 / 120, so the kernel must decide these itself; nearer ones it may hand back
            _add("%s, %s change: %s" % (name, which, what), 5, "device" if what.startswith("10000 ") else "any", lambda name=name, v=v: sweep_list(name, v))


def seeds_spent(w):
    """try_find_best_board takes its seeds from the fullest round(theta) bin, highest list position first, 30 at most.  The 7 x 7
    lattice first, then w - 5 far saddles of its seed bin (no quad), then a 3 x 3 lattice (one quad, five saddles of the bin):
    w seeds are spent before the 7 x 7 lattice's.  Its last saddle, a corner, is in no valid cell and its last but two seeds the
    nine quads: they are found if that one is among the 30, so with w <= 28, and with w = 29 the 3 x 3 lattice's quad is all."""
    far = far_saddles(w - 5, 77)
    far[:, 3] = 45.0
    return np.concatenate([lattice(7, 7), far, lattice(3, 3, origin=(1500.0, 1500.0))])


def dense(n, spacing, copies=1):
    return repeated(lattice(n, n, spacing=spacing), copies)


def unbalanced(n, m):
    """n x n where only every m-th diagonal has the first orientation, all of it in one theta bin (-45: the fullest bin, so the
    seeds), and the rest is spread over the bins 43 .. 47 (one orientation still): a seed's 50 nearest hold 33 (m = 3) or 37
    (m = 4) saddles of the other orientation -- 528 / 666 (d0, d1) pairs, more than TA3."""
    l = lattice(n, n)
    r, c = np.mgrid[0:n, 0:n]
    first = ((r + c) % m == 0).ravel()
    l[first, 3] = -45.0
    l[~first, 3] = 43.0 + (np.arange((~first).sum()) % 5)
    return l


def with_far(l, n, seed):
    return np.concatenate([l, far_saddles(n - len(l), seed)])


def _family6():
    # BGR = 12: a strip 2 x m has (m - 2) // 2 quads in a row; a cell is tried at +-(found cells + 1) of the seed's, and the
    # seed's place in the strip is the search's: the pair is pinned from the device
    for m in (20, 24, 26, 28, 30, 40):
        _add("strip 2x%d" % m if m != 30 else "lattice 2x30", 6, "limit-pair", lambda m=m: lattice(2, m, origin=(10.0, 60.0)), (m - 2) // 2)
    # BCELLS = 128 cells, found or not: n x n has about ((n - 1) / 2) ** 2 found ones and their not-found rim
    for n in (14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24):
        _add("lattice %dx%d" % (n, n), 6, "limit-pair", lambda n=n: lattice(n, n, origin=(10.0, 10.0)), 90 if n == 20 else -1)
    _add("lattice 32x32", 6, "any", lambda: lattice(32, 32, origin=(10.0, 10.0)), 240)  # 1024 saddles, and far more than BCELLS cells
    # TN = 1024 listed saddles: 1024 is the kernel's, 1025 the host's (tail_kernels.hip: n > TN), whatever the list shows
    _add("7x7 and far saddles, 1023 in all", 6, "limit-pair", lambda: with_far(lattice(7, 7), 1023, 1))
    _add("7x7 and far saddles, 1024 in all", 6, "limit-pair", lambda: with_far(lattice(7, 7), 1024, 2))
    _add("7x7 and far saddles, 1025 in all", 6, "limit-pair", lambda: with_far(lattice(7, 7), 1025, 3))
    _add("7x7 and far saddles, 1100 in all", 6, "limit-pair", lambda: with_far(lattice(7, 7), 1100, 4))
    _add("lattice 32x32 and a far saddle", 6, "any", lambda: with_far(lattice(32, 32, origin=(10.0, 10.0)), 1025, 5), 240)
    # TCAND = 256 candidate quads and TA3 = 512 (d0, d1) pairs of one seed: its 50 nearest hold many saddles of both orientations
    for sp in (2.0, 3.0, 4.0):
        _add("dense 9x9 spacing %g" % sp, 6, "device", lambda sp=sp: dense(9, sp))
        _add("dense 13x13 spacing %g" % sp, 6, "device", lambda sp=sp: dense(13, sp))
    # ... and copies: every saddle k times multiplies a seed's candidate quads by k^3
    for k in (4, 5, 6, 8):
        _add("7x7 every saddle %d times" % k, 6, "limit-pair", lambda k=k: repeated(lattice(7, 7), k), 2 if k == 4 else -1)
    for m in (2, 3, 4):
        _add("unbalanced 11x11, every %d. diagonal" % m, 6, "device", lambda m=m: unbalanced(11, m))
    # 30 seeds at most from the fullest theta bin
    for w, quads in ((27, 9), (28, 9), (29, 1), (30, 1)):
        _add("30 seeds: %d spent before the lattice's" % w, 6, "device", lambda w=w: seeds_spent(w), quads)


def _ties_in_other_orders():
    """Families 3 and 4 again under four seeded permutations and reversed: where distances tie exactly, the order of the list is
    all that decides."""
    for c in [c for c in CASES if c.family in (3, 4)]:
        for seed in range(4):
            _add("%s, perm %d" % (c.name, seed), c.family, "device", lambda c=c, seed=seed: permuted(c.build(), 200 + seed)[0])
        _add(c.name + ", reversed", c.family, "device", lambda c=c: c.build()[::-1].copy())


_family1()
_family2()
_family3()
_family4()
_ties_in_other_orders()
_family5()
_family6()
BY_NAME = {c.name: c for c in CASES}
FAMILIES = sorted({c.family for c in CASES})

# The straddling pairs.  TN follows from the constant (tail_kernels.hip: n > TN).  The other three depend on where the search's
# first seed lands and on how many candidate quads it has, so they are the statuses before the fetch of the first run on an
# MI355X, each read against the code:
#   BGR     a cell is tried at the seed's +-(cells in a row + 1); the seed of a strip is its first quad, so 12 quads in a row try
#           cell 12 (inside +-BGR) and 13 try cell 13 (build_board_w: nx > BGR);
#   BCELLS  20 x 20 has 90 found cells and a rim of not-found ones within 128, 21 x 21 (100 found) has more (n_cells == BCELLS);
#   TCAND   three copies of every saddle give a seed 27 times its candidate quads, four copies 64 times: beyond 256 (nc > TCAND).
PAIRS = [
    ("TN: more than 1024 listed saddles", ["7x7 and far saddles, 1023 in all", "7x7 and far saddles, 1024 in all"],
     ["7x7 and far saddles, 1025 in all", "7x7 and far saddles, 1100 in all"]),
    ("BGR: a board cell beyond +-12 of the seed's", ["strip 2x20", "strip 2x24", "strip 2x26"],
     ["strip 2x28", "lattice 2x30", "strip 2x40"]),
    ("BCELLS: more than 128 cells, found or not", ["lattice %dx%d" % (n, n) for n in (14, 15, 16, 17, 18, 19, 20)],
     ["lattice %dx%d" % (n, n) for n in (21, 22, 23, 24)]),
    ("TCAND: more than 256 candidate quads of one seed", ["7x7 every saddle 2 times", "7x7 every saddle 3 times"],
     ["7x7 every saddle %d times" % k for k in (4, 5, 6, 8)]),
]


def build(name):
    l = np.ascontiguousarray(BY_NAME[name].build(), F32)
    assert l.ndim == 2 and l.shape[1] == 5
    return l
