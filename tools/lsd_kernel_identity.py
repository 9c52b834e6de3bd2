#!/usr/bin/env python3
"""Compare the gfx950 code of the LSD kernels of two trees, kernel by kernel (no GPU needed), and list their resources.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S <tree>/stvo-pl_amd/csrc/lsd_kernels.hip -o <tree>.s     (both trees)
    python tools/lsd_kernel_identity.py parent.s this.s

A kernel is matched by its demangled name with the template arguments this change adds struck (lsd_grow_xcd_kernel<P> is
lsd_grow_xcd_kernel<P, false>); its body is every line between its label and its end label, with the kernel's own mangled name replaced,
so branch targets, instruction order and operands all count; an empty struct appended to the arguments shows as a longer argument block.  Prints one line per kernel: identical / DIFFERENT / new, and the
instruction count and resources of each (VGPRs, SGPRs, static LDS, scratch)."""
import re
import subprocess
import sys


def kernels(path):
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M):
        name, body = m.group(1), m.group(2)
        desc = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", txt, re.S)
        if not desc:
            continue
        res = {k: int(v) for k, v in re.findall(r"\.set " + re.escape(name) + r"\.(num_vgpr|num_agpr|numbered_sgpr|private_seg_size), (\d+)", txt)}
        res["lds"] = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc.group(1)).group(1))
        lines = [re.sub(r"\.L(BB|JTI)\d+_", r".L\1_", re.sub(r"\s*;.*$", "", l)).replace(name, "KERNEL") for l in body.splitlines()]  # (labels carry the function's number in the file)
        # (the match runs on into the kernel descriptor: its lines count too, but for the size of the argument block, reported apart)
        out[name] = ("\n".join(l for l in lines if l.strip() and not l.lstrip().startswith((".p2align", ".amdhsa_kernarg_size"))), res,
                     int(re.search(r"\.amdhsa_kernarg_size (\d+)", desc.group(1)).group(1)))
    return out


def demangle(names):
    p = subprocess.run(["c++filt"] + list(names), capture_output=True, text=True, check=True)
    return dict(zip(names, p.stdout.splitlines()))


def key(dem):
    """the kernel's name and template arguments, without the argument list; the parent's lsd_grow_xcd_kernel<P> is <P, false>"""
    k = re.sub(r"\(.*$", "", dem.replace("stvo::(anonymous namespace)::", "")).replace("void ", "")
    m = re.fullmatch(r"lsd_grow_xcd_kernel<(\w+)>", k)
    return "lsd_grow_xcd_kernel<%s, false>" % m.group(1) if m else k


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    da, db = demangle(list(a)), demangle(list(b))
    ka = {key(da[n]): a[n] for n in a}
    bad = 0
    for n in sorted(b, key=lambda n: key(db[n])):
        k = key(db[n])
        body, res, karg = b[n]
        n_ins = sum(1 for l in body.splitlines() if not l.lstrip().startswith(".") and not l.rstrip().endswith(":"))
        r = "instrs %4d  VGPR %3d  AGPR %d  SGPR %3d  LDS %6d  scratch %d" % (n_ins, res["num_vgpr"], res["num_agpr"], res["numbered_sgpr"], res["lds"], res["private_seg_size"])
        if k not in ka:
            verdict = "new"
        elif ka[k][0] == body and ka[k][1] == res:
            verdict = "identical (%d lines)" % len(body.splitlines())
            if ka[k][2] != karg:
                verdict += ", argument block %d -> %d bytes" % (ka[k][2], karg)
        else:
            verdict = "DIFFERENT"
            bad += 1
        print("%-52s %s   %s" % (k, r, verdict))
    missing = set(ka) - {key(db[n]) for n in b}
    for k in sorted(missing):
        print("%-52s gone" % k)
    return 1 if bad or missing else 0


if __name__ == "__main__":
    sys.exit(main())
