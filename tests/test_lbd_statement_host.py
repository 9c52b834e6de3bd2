"""The LBD oracle (oracle/stvo_lbd_oracle.c) against the plain statement (tests/np_lbd.py) on the planned key-lines of
tests/lbd_edge_cases.py, bit for bit, and every case's "this input really sits on its edge" facts.  No GPU.
tests/test_gpu_lbd_edges.py compares the kernels with the same statement: where they differ, this file says which side is wrong.

Float against exact (np_lbd's longdouble mode), measured on the planned set with the host's C library, NaN lines apart: the per-line
largest deviation of the 72 float components from the extended ones has a MEDIAN of 7.7e-8 (asserted at 4 x that: another
library's sqrt / cos in extended precision) and a MAXIMUM of 5.9e-7 (recorded, not bounded).  In 97 of the 123 lines, the maximum's among them, the
largest deviation sits in a standard-deviation component sqrt(sum c^2 r^2 / N - mean^2): the two terms cancel, the remainder keeps
their absolute error, and the square root of a small remainder magnifies it.  The closer a band is to uniform along its rows the
larger the figure, without a bound short of the component itself.  That is the reference's own arithmetic, not a defect of any
restatement.  Of the planned set's decided bits (exact ties and NaN lines apart) 1.1 %
have an extended margin |f1 - f2| below twice their line's deviation and are left out of the byte comparison; the cap is 5 %."""
import math

import numpy as np
import pytest

import lbd_edge_cases as ec
import np_lbd
from golden import gen_lbd_hard_angles as gen

CASES = {c["name"]: c for c in ec.all_cases() + ec.crop_cases() + [ec.hard_angle_lines()]}
MEDIAN_DEVIATION = 7.7e-8      # measured on the planned set (this file's docstring)


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def image_of(c, b):
    im = c["images"][b]
    return im if c["size"] is None else np.ascontiguousarray(im[:c["size"][1], :c["size"][0]])


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_equals_the_statement(oracle, name):
    c = CASES[name]
    for b, (n, e) in enumerate(zip(ec.counts(c), ec.expected(c))):
        d, f = oracle.lbd_compute(image_of(c, b), c["lines"][b][:n], c["npx"][b][:n], want_float=True)
        assert bits_equal(f, e["desc_f"]), (name, b)              # the 72 floats, NaN payloads included
        assert np.array_equal(d, e["desc"]), (name, b)


@pytest.mark.parametrize("name", list(CASES))
def test_case_sits_on_its_edge(name):
    c = CASES[name]
    c["facts"]([e["trace"] for e in ec.expected(c)])


def test_random_lines_of_the_existing_kind(oracle):
    from stvo_amd import synth
    from test_gpu_lbd import random_lines
    for cols, rows, n in ((64, 48, 120), (160, 120, 120), (259, 66, 120)):
        img = synth.make_image(40 + n, cols=cols, rows=rows, n_rects=60, n_discs=20)
        ln, npx = random_lines(np.random.default_rng(cols + n), n, cols, rows, len_px=(1.0, 150.0))
        e = np_lbd.compute(img, ln, npx)
        d, f = oracle.lbd_compute(img, ln, npx, want_float=True)
        assert bits_equal(f, e["desc_f"]) and np.array_equal(d, e["desc"]), (cols, rows)


def test_tables_blur_and_sobel_against_the_oracle(oracle):
    L, G = oracle.lbd_tables()
    sL, sG = np_lbd.tables()
    assert np.array_equal(L, sL) and np.array_equal(G, sG)
    for c in (CASES["smallest_image"], CASES["gradient_words"], CASES["launch_1_lines"]):
        img = c["images"][0]
        blur = np_lbd.gaussian_blur5(img)
        assert np.array_equal(oracle.gaussian_blur5(img), blur)
        dx, dy = np_lbd.sobel3(blur)
        odx, ody = oracle.sobel3(blur)
        assert np.array_equal(dx, odx) and np.array_equal(dy, ody)


def test_pair_rule():
    """The statement's rule against the kernel's form of it: band i pairs with the next cnt[i] bands."""
    cnt = [6, 5, 6, 5, 4, 3, 2, 1]
    assert np_lbd.pairs() == [(i, i + 1 + k) for i in range(8) for k in range(cnt[i])] and len(np_lbd.pairs()) == 32
    assert len(set(np_lbd.pairs())) == 32 and np_lbd.pairs(omit=False)[6] == (0, 7)


# the planned case (and its lines) that tells each near miss from the rule
WITNESS = {
    "round_half_even": ("rounding_ties", None),
    "clamp_cols": ("clamps_exact", None),
    "clamp_slot": ("clamps_each_border@crop", None),
    "swap_neighbour_weights": ("walk_lengths", None),
    "invn3_outer": ("walk_lengths", None),
    "binary_ge": ("statistics", None),
    "bit_reverse": ("walk_lengths", None),
    "pairs_all": ("walk_lengths", None),
    "no_short_cast": ("walk_wraps", [1, 4]),       # -3 and -65533 (a walk of 3); the lines of 32768 and 65537 steps would only take long
    "steps_minus_1": ("walk_lengths", None),
}


def mutated(c, switch, only=None):
    out = []
    for b, n in enumerate(ec.counts(c)):
        idx = list(range(n)) if only is None else only
        out.append((idx, np_lbd.compute(c["images"][b], c["lines"][b][idx], c["npx"][b][idx], size=c["size"], mutate=(switch,))))
    return out


@pytest.mark.parametrize("switch", list(WITNESS))
def test_every_near_miss_changes_a_planned_case(switch):
    name, only = WITNESS[switch]
    c = CASES[name]
    changed_f = changed_d = 0
    for (idx, m), e in zip(mutated(c, switch, only), ec.expected(c)):
        changed_f += int(not bits_equal(m["desc_f"], e["desc_f"][idx]))
        changed_d += int(not np.array_equal(m["desc"], e["desc"][idx]))
    if switch in ("binary_ge", "bit_reverse", "pairs_all"):
        assert changed_d > 0 and changed_f == 0, (switch, name)   # rules of the 32 bytes: the 72 floats stay
    else:
        assert changed_f > 0, (switch, name)


def test_the_clip_comparison_cannot_show():
    """`>=` for `>` in the 0.4 clip — like a comparison in float, 0.4f against 0.4 — is the one near miss no input can show: the only
    component on which the two differ is 0.4f itself, and the clip writes 0.4f over it.  Asserted as what it is: the switch changes
    no output on any planned case."""
    assert float(np.float32(0.4)) > 0.4
    for c in ec.all_cases():
        for (idx, m), e in zip(mutated(c, "clip_ge"), ec.expected(c)):
            assert bits_equal(m["desc_f"], e["desc_f"]) and np.array_equal(m["desc"], e["desc"]), c["name"]
    assert set(WITNESS) | {"clip_ge"} == set(np_lbd.MUTATIONS)


def test_round_away_at_the_float_below_a_half():
    x = np.array([0.49999997, 0.5, -0.5, 1.5, 2.5, -2.5, 8388609.0], np.float32)
    assert np_lbd.round_away(x).tolist() == [0, 1, -1, 2, 3, -3, 8388609]


def test_extended_precision_bytes_and_deviation(oracle):
    """np_lbd's longdouble mode on the planned set (the module's docstring holds the figures)."""
    dev, left_out, decided = [], 0, 0
    for c in ec.all_cases():
        for b, n in enumerate(ec.counts(c)):
            if n == 0:
                continue
            x = np_lbd.compute(c["images"][b], c["lines"][b][:n], c["npx"][b][:n], dtype=np.longdouble)
            assert bits_equal(x["desc_f"], ec.expected(c)[b]["desc_f"])
            orc = oracle.lbd_compute(c["images"][b], c["lines"][b][:n], c["npx"][b][:n])
            ok = ~np.isnan(x["deviation"].astype(np.float64))              # NaN lines apart
            obits = np.unpackbits(orc[ok][:, :, None], axis=2, bitorder="little").astype(bool)
            margin, d = x["margin"][ok], x["deviation"][ok]
            f = ec.expected(c)[b]["desc_f"][ok]
            pr = np_lbd.pairs()
            tie = np.stack([f[:, 8 * i:8 * i + 8] == f[:, 8 * j:8 * j + 8] for i, j in pr], 1)   # exact ties of the float descriptor apart
            sure = margin > 2 * d[:, None, None]
            assert np.array_equal(x["bits"][ok][sure], obits[sure]), (c["name"], b)
            decided += int((~tie).sum())
            left_out += int((~sure & ~tie).sum())
            dev += [float(v) for v in d]
    dev = np.array(dev)
    print(f"lines {len(dev)}  deviation median {np.median(dev):.3g} max {dev.max():.3g}  bits left out {left_out} of {decided} = {left_out / decided:.4f}")
    assert left_out <= 0.05 * decided
    assert np.median(dev) <= 4 * MEDIAN_DEVIATION


def test_hard_angle_fixture():
    """Every row re-derived; one seeded block of 2^22 floats, and the block of the fixture's last row, swept again: exactly the fixture's rows."""
    h = ec.hard_angles()
    assert len(h["angle"]) > 0 and np.all(h["angle"] >= 0) and np.all(h["angle"] <= np.float32(math.pi))
    for a, fn, off, b in zip(h["angle"], h["fn"], h["offset"], h["bits"]):
        v = (math.cos, math.sin)[fn](float(a))
        assert int(gen.offsets([v])[0]) == int(off) and abs(int(off)) <= gen.WINDOW and gen.libm_bits(a, fn) == int(b)
    rows = list(zip(h["angle"].view(np.uint32).tolist(), h["fn"].tolist(), h["offset"].tolist(), h["bits"].tolist()))
    assert rows == sorted(rows) and len(set(rows)) == len(rows)
    seeded = int(np.random.default_rng(2022).integers(gen.N_BLOCKS))
    for k in {seeded, rows[-1][0] // gen.BLOCK}:
        assert gen.sweep_block(k) == [r for r in rows if r[0] // gen.BLOCK == k], k
