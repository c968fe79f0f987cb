"""Static guard on the code the compiler makes of the bit-exact two-column kernel's EARLY form.

The twelve row sums the EARLY form computes in the wave's low-priority phase are written term-major in fold_ab(), so
that consecutive instructions belong to different dependency chains.  Written chain by chain, the compiler ran all 72
packed instructions through one register pair with a hazard wait state behind every link (90 and 76 `s_nop` per two
rows of the two instantiations below).  Nothing at run time shows that -- the bits are the same either way -- so the
assembly is checked here: no scratch, the two-wave register footprint, exactly the arithmetic there was, and no more
wait states than the non-EARLY form has (28 per two rows).

CPU only: the kernels are compiled device-only to assembly with the Makefile's HIPFLAGS and parsed the way
tools/isa_mix.py does.  Skipped where there is no hipcc.
"""
import collections
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ssim_amd", "csrc", "ssim_kernels.hip")

MAX_VGPRS = 232         # the two-wave footprint ssim_probe.hip pads to
PACKED_PER_TWO_ROWS = 552
MAX_S_NOP = 28          # what the non-EARLY form <0,0,false,false> has per two rows

# ssim_strip2_kernel<MODE_EXACT, MAP, EARLY, BAL>: the headline's kernel, and the one 8192^2 pairs with a map run
KERNELS = {"<0,0,true,true>": "ssim_strip2_kernelILi0ELi0ELb1ELb1EE", "<0,2,true,false>": "ssim_strip2_kernelILi0ELi2ELb1ELb0EE"}


def _makefile_hipcc_and_flags():
    """HIPCC and HIPFLAGS as `make lib` uses them (default flavour: DOUBLE unset)."""
    var = {}
    with open(os.path.join(ROOT, "Makefile")) as f:
        for line in f:
            m = re.match(r"^(\w+)\s*[:?]?=\s*(.*)$", line.rstrip("\n"))
            if m and m.group(1) not in var:
                var[m.group(1)] = m.group(2).strip()
    flags = re.sub(r"\$\(if \$\(DOUBLE\),[^)]*\)", "", var["HIPFLAGS"])
    flags = re.sub(r"\$\((\w+)\)", lambda m: var[m.group(1)], flags)
    return os.environ.get("HIPCC", var["HIPCC"]), flags.split()


def _hot_loop_mix(body):
    """Instruction counts of the innermost loop with the most FMAs (the main two-row loop), spans found as tools/isa_mix.py finds them."""
    lines = body.split("\n")
    lab = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            lab[m.group(1)] = i
    isfma = [1 if re.match(r"\s*v_(pk_)?fma(c)?_f(32|64)", l) else 0 for l in lines]
    total = max(sum(isfma), 1)
    spans = []
    for i, l in enumerate(lines):
        m = re.search(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in lab and lab[m.group(1)] < i:
            span = (lab[m.group(1)], i)
            if sum(isfma[span[0]:span[1]]) >= 0.1 * total:
                spans.append(span)
    spans = [sp for sp in spans if not any(o != sp and sp[0] <= o[0] and o[1] <= sp[1] for o in spans)]
    assert spans, "no loop found"
    hot = max(spans, key=lambda sp: sum(isfma[sp[0]:sp[1]]))
    c = collections.Counter()
    for l in lines[hot[0]:hot[1] + 1]:
        l = l.strip()
        if not l or l[0] in ";." or l.endswith(":"):
            continue
        c[l.split()[0]] += 1
    return c


def parse_kernels(asm):
    """{mangled name: {"vgprs", "scratch", "packed", "valu", "s_nop"}} of every ssim_strip2_kernel in a device assembly file."""
    out = {}
    starts = [(m.start(), m.group(1)) for m in re.finditer(r"^(_ZN8ssim_hip\S*):", asm, re.M)]
    for idx, (pos, name) in enumerate(starts):
        if "ssim_strip2_kernel" not in name:
            continue
        end = starts[idx + 1][0] if idx + 1 < len(starts) else len(asm)
        c = _hot_loop_mix(asm[pos:end])
        desc = re.search(r"^\s*\.amdhsa_kernel " + re.escape(name) + r"\s*$(.*?)^\s*\.end_amdhsa_kernel", asm, re.M | re.S).group(1)
        out[name] = {
            "vgprs": int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)),
            "scratch": int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)),
            "packed": sum(v for k, v in c.items() if k.startswith("v_pk_")),
            "valu": sum(v for k, v in c.items() if k.startswith("v_")),
            "s_nop": c["s_nop"],
        }
    return out


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    hipcc, flags = _makefile_hipcc_and_flags()
    if not os.path.exists(hipcc) and shutil.which(hipcc) is None:
        pytest.skip("no hipcc: the kernels' assembly cannot be produced")
    out = str(tmp_path_factory.mktemp("isa") / "ssim_kernels.s")
    r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", SRC, "-o", out], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(out) as f:
        return parse_kernels(f.read())


@pytest.mark.parametrize("form", sorted(KERNELS))
def test_early_form_is_interleaved(kernels, form):
    match = [k for k in kernels if KERNELS[form] in k]
    assert len(match) == 1, (form, sorted(kernels))
    k = kernels[match[0]]
    print(form, k)
    assert k["scratch"] == 0, k
    assert k["vgprs"] <= MAX_VGPRS, k
    assert k["packed"] == PACKED_PER_TWO_ROWS, k        # no arithmetic added or lost
    assert k["s_nop"] <= MAX_S_NOP, k
