"""Which search kernel an LSD detection launches (stvo-pl_amd/csrc/lsd_route.h), run on the host through tests/cpp/lsd_route_host.cpp
over every combination of its facts: against a plain statement of the rule written here, and — with no table, or with the table route at
its default — against the chain of conditions lsd_enqueue held before the header existed, transcribed below.  No GPU."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cpp", "lsd_route_host.cpp")
HDR = os.path.join(ROOT, "stvo-pl_amd", "csrc", "lsd_route.h")
NEW_SYMBOLS = ("stvo_lsd_set_table_route", "stvo_lsd_search_route")

ONE_WAVE, PLAIN, MANY = 0, 1, 2
TABLE_ONE_WAVE, TABLE_BY_BATCH = 0, 1
# refine (2: a value the detector refuses at creation, taken as "not 1"), arena, table, table route, STVO_LSD_GROW (unset is 1), probes
FACTS = list(itertools.product((0, 1, 2), (0, 1), (0, 1), (TABLE_ONE_WAVE, TABLE_BY_BATCH), (0, 1, 7), (0, 1)))


@pytest.fixture(scope="module")
def lrh():
    so = os.path.join(HERE, "cpp", "liblsd_route_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in (SRC, HDR)):
        tmp = "%s.%d.so" % (so[:-3], os.getpid())
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", tmp, SRC])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.lrh_route.argtypes = [C.c_int] * 6
    lib.lrh_values.argtypes = [np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")]
    return lib


def decide(lib, f):
    v = lib.lrh_route(*f)
    return v & 0xFF, bool(v >> 8 & 1), bool(v >> 9 & 1)


def statement(refine, arena, table, table_route, lsd_grow, probes):
    """the rule in plain words: refinement owns its kernel; a detector with the arena runs many waves unless a table under the default
    table route forbids it; the cross-check switch picks the plain form of what is left.  The probe instances: no table, no refinement."""
    if refine == 1:
        search = PLAIN
    elif arena and not (table and table_route == TABLE_ONE_WAVE):
        search = MANY
    else:
        search = PLAIN if lsd_grow == 0 else ONE_WAVE
    return search, refine == 1, bool(probes) and not table and refine != 1


def parent_chain(refine, wdev, n_sizes, lsd_grow, dbg):
    """lsd_enqueue before this header: the kernel each branch launched, (search, REFINE instance, PROF instance)"""
    if n_sizes:
        if refine == 1:
            return PLAIN, True, False      # lsd_grow_refine_kernel<true, false, true>
        elif lsd_grow == 0:
            return PLAIN, False, False     # lsd_grow_refine_kernel<false, false, true>
        else:
            return ONE_WAVE, False, False  # lsd_grow_kernel<false, true>
    prof = bool(dbg)
    if refine == 1:
        return PLAIN, True, False          # lsd_grow_refine_kernel<true, false, false>
    elif wdev:
        return MANY, False, prof           # lsd_grow_xcd_kernel<prof>
    elif lsd_grow == 0:
        return PLAIN, False, prof          # lsd_grow_refine_kernel<false, prof, false>
    else:
        return ONE_WAVE, False, prof       # lsd_grow_kernel<prof, false>


def test_values_are_the_public_ones(lrh):
    from stvo_amd import capi
    v = np.zeros(5, np.int32)
    lrh.lrh_values(v)
    assert v.tolist() == [ONE_WAVE, PLAIN, MANY, TABLE_ONE_WAVE, TABLE_BY_BATCH]
    assert v.tolist() == [capi.LSD_SEARCH_ONE_WAVE, capi.LSD_SEARCH_ONE_WAVE_PLAIN, capi.LSD_SEARCH_MANY_WAVES, capi.LSD_TABLE_ONE_WAVE,
                          capi.LSD_TABLE_BY_BATCH]
    hdr = open(os.path.join(ROOT, "include", "stvo_hip.h")).read()
    for name, val in zip(("SEARCH_ONE_WAVE", "SEARCH_ONE_WAVE_PLAIN", "SEARCH_MANY_WAVES", "TABLE_ONE_WAVE", "TABLE_BY_BATCH"), v.tolist()):
        assert re.search(r"#define STVO_LSD_%s %d\b" % (name, val), hdr), name
    assert [lrh.lrh_table_route_ok(r) for r in (-1, 0, 1, 2, 1 << 30)] == [0, 1, 1, 0, 0]


def test_every_combination_against_the_statement(lrh):
    assert len(FACTS) == 3 * 2 * 2 * 2 * 3 * 2
    for f in FACTS:
        assert decide(lrh, f) == statement(*f), f
    # the rule does what it is for: some combination reaches each kernel, and the table route matters exactly where a table is in force
    # on a detector with the arena and no refinement
    assert {decide(lrh, f)[0] for f in FACTS} == {ONE_WAVE, PLAIN, MANY}
    for refine, arena, table, _, grow, probes in FACTS:
        a = decide(lrh, (refine, arena, table, TABLE_ONE_WAVE, grow, probes))
        b = decide(lrh, (refine, arena, table, TABLE_BY_BATCH, grow, probes))
        assert (a != b) == bool(arena and table and refine != 1), (refine, arena, table, grow, probes)
        if a != b:
            assert b[0] == MANY and a[0] in (ONE_WAVE, PLAIN)


def test_no_table_and_the_default_route_are_the_chain_as_it_was(lrh):
    for refine, arena, table, table_route, grow, probes in FACTS:
        if table and table_route != TABLE_ONE_WAVE:
            continue
        assert decide(lrh, (refine, arena, table, table_route, grow, probes)) == parent_chain(refine, arena, table, grow, probes), \
            (refine, arena, table, table_route, grow, probes)
    # and with no table the table route is not looked at
    for refine, arena, _, _, grow, probes in FACTS:
        assert decide(lrh, (refine, arena, 0, TABLE_BY_BATCH, grow, probes)) == parent_chain(refine, arena, 0, grow, probes)


def test_header_declares_and_library_exports_the_new_symbols():
    from stvo_amd import capi
    hdr = open(os.path.join(ROOT, "include", "stvo_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    lib = capi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in capi.EXPORTS and hasattr(lib, name), name
