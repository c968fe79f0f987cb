#!/usr/bin/env python3
"""tests/golden/ref_outputs.json: what the REAL reference returns on the inputs of tests/test_oracle_vs_ref.py, and the macro
surface of the reference's public header (tests/test_abi_cpu.py), recorded so that those tests run without the reference tree.

Runs ONLY where the reference tree is present (oracle/_ref built from it, and its include/ directory for the macro dump).
What it writes is data: float bits, fp64 sums and sha256 digests of maps and of the preprocessor's macro dump.  No reference
source text is stored.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle as o                  # noqa: E402
import test_abi_cpu as abi          # noqa: E402
import test_oracle_vs_ref as ovr    # noqa: E402

REF_INCLUDE = "/root/reference/include"
OUT = os.path.join(ROOT, "tests", "golden", "ref_outputs.json")


def main():
    import pathlib
    import tempfile
    assert o.have_ref() and os.path.isdir(REF_INCLUDE), "needs oracle/_ref and the reference tree"
    out = {"_about": "reference outputs on the inputs of tests/test_oracle_vs_ref.py and the macro surface of its header; tests/tools/make_ref_outputs.py",
           "random_images": {}, "flat_images": [], "naive_f64": None, "macro_surface": {}}
    for impl in (5, 4):
        out["random_images"][str(impl)] = [ovr.digest(*o.ref_ssim(a, b, want_map=True, impl=impl)) for a, b in ovr.random_pairs()]
    out["flat_images"] = [ovr.digest(*o.ref_ssim(a, b, want_map=True)) for a, b in ovr.flat_pairs()]
    a, b = ovr.naive_pair()
    rv, rm = o.ref_naive_f64(a, b, want_map=True)
    out["naive_f64"] = ovr.digest(rv, rv, rm)
    a, b = o.synth_pair(1920, 1080, 0x5EED)
    out["openmp_1080p_5eed"] = {str(t): ovr.digest(*o.ref_ssim(a, b, threads=t))["ssim_hex"] for t in (1, 8)}
    tmp = pathlib.Path(tempfile.mkdtemp())
    for cc in abi.MACRO_SURFACE_CCS:
        if "/" in cc.split()[0] and not os.path.exists(cc.split()[0]):
            continue
        dump = abi._macro_dump(REF_INCLUDE, cc, tmp, "ref")
        pre = abi._predefined(cc)
        family = [f for f in abi.VERSION_MACRO_FAMILIES if [pre.get(m) for m in f] == abi._version_values(dump)]
        assert len(family) == 1, (cc, abi._version_values(dump))
        out["macro_surface"][cc] = {"compiler": abi._compiler_version(cc), "lines": len(dump),
                                    "sha256": abi._macro_sha(dump), "sha256_without_version_values": abi._macro_sha(dump, versions=False), "version_macros": list(family[0])}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
