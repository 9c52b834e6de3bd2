"""Generator of tests/golden/lbd_hard_angles.npz: the float directions at which two correct C libraries may disagree about
(float) cos((double) a) or (float) sin((double) a) — what lbd_describe_kernel takes from the device's library and
oracle/stvo_lbd_oracle.c from the host's.

A double rounds to one of two floats according to its low 29 mantissa bits: below the midpoint pattern 2^28 it rounds down, above it
up.  Two libraries that each err by less than one unit in the last place of the double can fall on different sides only where the
double sits within 2 units of that pattern.  The window kept here is twice that, |low 29 bits - 2^28| <= 4: stated, not measured.

The sweep takes every float in [0, pi] (1 078 530 012 of them; cos is even and sin is odd, so the negative half follows by symmetry)
in blocks of 2^22 consecutive bit patterns, a minute or two on one core:
    python tests/golden/gen_lbd_hard_angles.py
The sweep finds 5 rows.  That is what the window predicts: below about 2^-12 the double is too close to a float (cos to 1, sin to
the angle itself) to reach a midpoint at all, which leaves 1.1e8 floats, two functions and a chance of 9 / 2^29 each: about 4.
Rows: angle (float32), fn (0: cos, 1: sin), offset (the low 29 bits minus 2^28), bits (the double, as the C library here returns it)."""
import math
import os
import struct

import numpy as np

BLOCK = 1 << 22
WINDOW = 4
LAST = int(np.float32(math.pi).view(np.uint32))            # 0x40490FDB, the float nearest pi (just above it)
N_BLOCKS = LAST // BLOCK + 1
MID, MASK = 1 << 28, (1 << 29) - 1


def offsets(d):
    """low 29 mantissa bits of doubles minus the midpoint pattern"""
    return (np.asarray(d, np.float64).view(np.uint64) & np.uint64(MASK)).astype(np.int64) - MID


def sweep_block(k):
    """the hard rows of block k: (angle float32, fn, offset, bits) sorted by angle, cos before sin"""
    lo, hi = k * BLOCK, min((k + 1) * BLOCK, LAST + 1)
    a32 = np.arange(lo, hi, dtype=np.uint32).view(np.float32)
    a = a32.astype(np.float64)
    rows = []
    for fn, f in ((0, np.cos), (1, np.sin)):
        v = f(a)
        off = offsets(v)
        for i in np.nonzero(np.abs(off) <= WINDOW)[0]:
            rows.append((int(a32[i].view(np.uint32)), fn, int(off[i]), int(v[i:i + 1].view(np.uint64)[0])))
    rows.sort()
    return rows


def libm_bits(angle, fn):
    """the double the C library's cos / sin returns for a float angle, as an integer"""
    v = (math.cos, math.sin)[fn](float(angle))
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def pack(rows):
    return dict(angle=np.array([r[0] for r in rows], np.uint32).view(np.float32), fn=np.array([r[1] for r in rows], np.uint8),
                offset=np.array([r[2] for r in rows], np.int8), bits=np.array([r[3] for r in rows], np.uint64))


def main():
    rows = []
    for k in range(N_BLOCKS):
        rows += sweep_block(k)
        if k % 32 == 0:
            print(f"block {k} / {N_BLOCKS}: {len(rows)} rows", flush=True)
    t = pack(rows)
    for a, fn, b in zip(t["angle"], t["fn"], t["bits"]):     # the vector functions of numpy and the scalar ones of the C library agree here
        assert libm_bits(a, fn) == int(b), (a, fn)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lbd_hard_angles.npz")
    np.savez(out, **t)
    print(f"{len(rows)} rows -> {out}")


if __name__ == "__main__":
    main()
