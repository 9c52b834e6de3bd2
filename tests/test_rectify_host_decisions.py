"""The host-side decisions of the rectify / colour entry points, without a GPU (tests/cpp/rectify_host_decisions.cpp, a stand-alone program
built by g++ alone under AddressSanitizer and UBSan): the chunking rule the uniform launch now shares with the rectifier bank
(rectify_bank_plan.h) gives the uniform launch's own grid for every (quad blocks 1 .. 2048, n 1 .. 600); gray_weights gives the four
documented weight sets and refuses every other (order, weights); the two range checks of rectify_internal.h accept and refuse a table
of touching, nested and disjoint ranges, the one-byte overlaps at either end included."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
SRC = os.path.join(HERE, "cpp", "rectify_host_decisions.cpp")
# rectify_internal.h includes the HIP headers; g++ reads them in host mode and nothing of the runtime is called or linked
FLAGS = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include")]


def test_stand_alone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "rectify_host_decisions")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + FLAGS + ["-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("0 failures"), out.stdout


def test_the_duplicated_items_are_defined_once():
    """What the three files used to state side by side has one definition under csrc/."""
    csrc = os.path.join(HERE, "..", "stvo-pl_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in os.listdir(csrc) if f.endswith((".hip", ".h", ".cpp"))}
    for needle in ("uint32_t blend(", "bool gray_weights(", "INSIDE = 0x8000u", "struct GrayWeights", "void load_px(", "void tap_px(",
                   "uint32_t weigh(", "bool stereo_ranges_ok(", "bool gray_planes_ok("):
        where = [f for f, t in text.items() if needle in t]
        assert len(where) == 1 and where[0] in ("rectify_px.h", "rectify_internal.h"), (needle, where)
    for f in ("rectify_kernels.hip", "color_kernels.hip"):
        assert "256 * 8" not in text[f] and (f == "rectify_kernels.hip" or "rbank_chunks(" in text[f])
    assert "rectify_remap_kernel" not in "".join(text.values())
