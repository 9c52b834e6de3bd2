"""The rectifier bank at the boundary, without a GPU: every stvo_rectify_bank_* symbol is declared in include/stvo_hip.h, listed in
capi.EXPORTS, exported by the library and bound with a ctypes signature that loads; capi.RectifierBank has the members the pipeline
uses."""
import ctypes as C
import inspect
import os
import re

from stvo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"stvo_rectify_bank_create": 7, "stvo_rectify_bank_destroy": 1, "stvo_rectify_bank_camera": 3, "stvo_rectify_bank_assign": 2,
         "stvo_rectify_bank_images_dev": 7, "stvo_rectify_bank_color_to_gray_dev": 11}   # arguments of each


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "stvo_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = capi.load()
    for name, nargs in NAMES.items():
        m = re.search(r"\bint %s\s*\((.*?)\);" % name, hdr, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert name in capi.EXPORTS and hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
    # a NULL bank is refused by the argument check alone (no device is touched)
    assert lib.stvo_rectify_bank_assign(None, None) == -1
    assert lib.stvo_rectify_bank_images_dev(None, 1, 1, None, None, None, None) == -1
    assert lib.stvo_rectify_bank_color_to_gray_dev(None, 1, 3, 0, 0, None, None, None, None, None, None) == -1
    assert lib.stvo_rectify_bank_camera(None, 0, None) == -1
    out = C.c_void_p()
    assert lib.stvo_rectify_bank_create(None, 1, 8, 8, None, 1, C.byref(out)) == -1 and not out.value
    assert lib.stvo_rectify_bank_destroy(None) == 0


def test_python_members():
    for name in ("assign", "camera", "rectify_dev", "rectify_color_to_gray_dev", "rectify", "rectify_color", "close"):
        assert callable(getattr(capi.RectifierBank, name)), name
    from stvo_amd import images
    assert "calibs" in inspect.signature(images.ImagePipeline.__init__).parameters
    assert "calibs" in inspect.signature(images.ImagePipeline.enqueue).parameters
    assert "calibs" in inspect.signature(images.ImagePipeline.push_images).parameters


def test_the_header_says_who_owns_the_maps():
    hdr = open(os.path.join(ROOT, "include", "stvo_hip.h")).read()
    at = hdr.index("stvo_rectify_bank stvo_rectify_bank;")
    assert "outlive" in hdr[at - 1200:at]


def test_the_plan_header_is_the_only_statement_of_the_split():
    src = open(os.path.join(ROOT, "stvo-pl_amd", "csrc", "rectify_bank.hip")).read()
    assert '#include "rectify_bank_plan.h"' in src and "plan_rectify_bank(" in src and "rbank_max_items(" in src
    mk = open(os.path.join(ROOT, "stvo-pl_amd", "Makefile")).read()
    assert "csrc/rectify_bank.hip" in mk and "csrc/rectify_bank_plan.h" in mk
