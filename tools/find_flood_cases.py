#!/usr/bin/env python3
"""Search of the sine_frame family (tests/shape_cases.py) for frames whose candidate components sit at the limits of the two
flood windows, and a greedy cover of every class tests/test_shape_cases_cpu.py asserts.  CPU only (the oracle); prints the
FLOOD_CASES table to paste into tests/shape_cases.py.

  python tools/find_flood_cases.py            # about a minute on 8 cores
"""
import os
import sys
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import shape_cases as S  # noqa: E402

H, W = 160, 256
THETAS = (0.3, 0.5, 0.78, 1.1, -0.5, -1.0)
RATIOS = (1.0, 2.4, 4.0)


def required_keys():
    req = {("beyond_only", "L"), ("beyond_only", "R"), ("beyond_only", "D"), ("beyond", "L"), ("beyond", "R"), ("beyond", "D"), ("second", "sh", 0), ("second", "sh", 31),
           ("second", "left_padding"), ("second", "right_padding"), ("second", "bottom_padding")}
    req |= {("L", v) for v in (13, 14, 15, 16, 17, 63, 64)} | {("R", v) for v in (13, 14, 15, 16, 17, 62, 63)}
    req |= {("D", v) for v in (29, 30, 61, 62)}
    return req


def classes(case):
    fmt, h, w = case[:3]
    return case, S.flood_classes(S.components(S.make_case(case)), h, w)


def alignment_done(found, f, v):
    return sum(1 for a in range(4) if (f, v, "sx&3", a) in found) >= 3


def main():
    cases = []
    px = 20.0  # (below the issue's 30: the frames whose components all stay in the first tier)
    while px <= 110.0:
        for th in THETAS:
            for ratio in RATIOS:
                cases.append(("L16", H, W, px, px * ratio, th, 0, 0))
        px += 1.5
    cases += [("L16", H, W, 64.25, 257.0, 1.1, 0, 0)]
    pool = {}
    with ProcessPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        for case, keys in ex.map(classes, cases, chunksize=16):
            pool[case] = keys
        # whole-pixel translations of every frame that reaches something: alignments sx & 3 and (sy - 1) & 31, borders
        useful = [c for c, k in pool.items() if k - {("all_first_tier",)}]
        shifted = [c[:6] + (ox, oy) for c in useful for ox in range(4) for oy in (0, 5, 11, 14, 19, 23, 28)
                   if (ox, oy) != (0, 0)]
        for case, keys in ex.map(classes, shifted, chunksize=16):
            pool[case] = keys
    req = required_keys()
    chosen, found = [], set()

    def gain(keys):
        g = len((keys & req) - found)
        for k in keys - found:
            if len(k) == 4 and not alignment_done(found, k[0], k[1]):
                g += 1
        return g

    while True:
        best = max(pool, key=lambda c: (gain(pool[c]), -abs(c[6]) - abs(c[7])))
        if gain(pool[best]) == 0:
            break
        chosen.append(best)
        found |= pool[best]
    small = sorted((c for c, k in pool.items() if ("all_first_tier",) in k and c[6:] == (0, 0)), key=lambda c: -c[3])
    chosen += [small[0], small[len(small) // 2]]
    # the same geometry in the other formats: the second-tier / generic frames that cover most, as L8 and LF32
    missing = sorted(req - found) + [(f, v) for f in "LR" for v in (13, 14, 15, 16, 17) if not alignment_done(found, f, v)]
    print("# %d frames searched; missing: %s" % (len(pool), missing or "nothing"))
    print("FLOOD_CASES = [")
    for c in chosen:
        print("    (%r, %d, %d, %r, %r, %r, %d, %d),  # %s" % (c + (" ".join(
            "".join(str(p) for p in k[:2]) if len(k) == 2 else ":".join(str(p) for p in k) for k in sorted(pool[c], key=str) if len(k) < 4),)))
    print("]")


if __name__ == "__main__":
    main()
