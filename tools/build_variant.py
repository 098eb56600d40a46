#!/usr/bin/env python
"""Build a second copy of libmsml_hip.so with extra -D flags on EVERY source file:
    python tools/build_variant.py --all MSML_LDS_GUARD -> variants/libmsml_MSML_LDS_GUARD.so
Select it at run time with MSML_LIB=<path> (msml_amd/_lib.py).  Used for the LDS high-water guard build
(msml_amd/csrc/common.h, MSML_LDS_REGION; tools/lds_guard_quick.sh runs it)."""
import concurrent.futures
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def build_all(defs):
    """Every source with the extra defines (e.g. MSML_LDS_GUARD): variants/libmsml_<tag>.so"""
    tag = "_".join(d.replace("=", "") for d in defs)
    outdir = os.path.join(ROOT, "variants", "obj_" + tag)
    os.makedirs(outdir, exist_ok=True)
    srcs = sorted(f for f in os.listdir(ge.CSRC) if f.endswith(".hip"))

    def cc(f):
        obj = os.path.join(outdir, f + ".o")
        subprocess.run([ge.HIPCC] + ge.FLAGS + ["-D" + d for d in defs] + ["-c", os.path.join(ge.CSRC, f), "-o", obj], check=True)
        return obj
    with concurrent.futures.ThreadPoolExecutor(max_workers=6) as ex:
        objs = list(ex.map(cc, srcs))
    lib = os.path.join(ROOT, "variants", "libmsml_%s.so" % tag)
    subprocess.run([ge.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs, check=True)
    print(lib)


def main():
    if len(sys.argv) < 3 or sys.argv[1] != "--all":
        raise SystemExit(__doc__)
    build_all(sys.argv[2:])


if __name__ == "__main__":
    main()
