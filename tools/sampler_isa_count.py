#!/usr/bin/env python3
"""What the search service's sampler of a ray's first batches issues (usage: sampler_isa_count.py [--csrc DIR] [extra hipcc flags ...]).

Cross-compiles smh_lsd.hip with the Makefile's flags and, for every callee of k_lsd_service / k_lsd_service_c that casts rays
(svc_frame, svc_frame_global, svc_help, svc_help_remote), finds the code that samples the candidate window (LSD_MODE_WIN2): the
instructions from the header of the loop that issues a batch's window reads to the branch behind its last whiteness bit (a
`v_alignbit_b32 vA, vB, vA, 1`); one ds_read_b32 is one sample; the index reads of the tile store (ds_read_u16, ds_read_b128) tell the long rays' sampler
apart, which is not counted.  Prints, per 16 samples: VALU (v_*), DS (ds_*), s_waitcnt and other SALU (s_*) instructions, counted
by mnemonic prefix only, and each kernel's VGPR and scratch figures as the compiler reports them.  --csrc: the csrc directory of
another checkout (the parent's, for the before / after)."""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
args = sys.argv[1:]
csrc = os.path.join(HERE, "..", "squad-mortar-helper_amd", "csrc")
if args[:1] == ["--csrc"]:
    csrc, args = args[1], args[2:]
CALLEES = r"svc_frameILb|svc_frame_globalILb|svc_helpILb|svc_help_remoteILb"
KERNELS = ("k_lsd_service", "k_lsd_service_c", "k_lsd_tile", "k_lsd")
BIT = re.compile(r"\s*v_alignbit_b32 (v\d+), v\d+, (v\d+), 1\s*$")
GAP = 150                                                   # lines between two whiteness bits of one batch, at the most


def compile_asm():
    out = subprocess.run(["make", "-pn", "-C", csrc, "print-nothing"], capture_output=True, text=True).stdout
    arch = re.search(r"^ARCH \??:?= (.*)$", out, re.M).group(1).strip()
    flags = re.search(r"^FLAGS :?= (.*)$", out, re.M).group(1).replace("$(ARCH)", arch).split()
    with tempfile.TemporaryDirectory() as tmp:
        s = os.path.join(tmp, "o.s")
        p = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + args + ["-x", "hip", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, "smh_lsd.hip"), "-o", s],
                           capture_output=True, text=True)
        if p.returncode != 0:
            sys.exit(p.stderr[-4000:])
        return open(s).read().split("\n"), p.stderr


def kernel_figures(remarks):
    fig, cur = {}, None
    for ln in remarks.splitlines():
        m = re.search(r"remark: Function Name: _ZN3smh\d+(\w+?)E(?:NS|P|v|$)", ln)
        if m:
            cur = m.group(1) if m.group(1) in KERNELS else None
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur:
            fig.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    return fig


def classify(line):
    op = line.split()[0] if line.split() else ""
    if op.startswith("s_waitcnt"):
        return "waits"
    for prefix, what in (("v_", "valu"), ("ds_", "ds"), ("s_", "salu")):
        if op.startswith(prefix):
            return what
    return None


def samplers(body):
    """(first line, last line, samples) of every window sampler in a function's lines"""
    bits = [k for k, l in enumerate(body) if (lambda m: m and m.group(1) == m.group(2))(BIT.match(l))]
    clusters = []
    for k in bits:
        if clusters and k - clusters[-1][-1] <= GAP:
            clusters[-1].append(k)
        else:
            clusters.append([k])
    out = []
    for c in clusters:
        # back from the first bit to the header of the loop around it: the batch's first reads are issued from there on
        start = c[0]
        while start > 0 and not (re.match(r"^\.LBB\d+_\d+:", body[start]) and "Loop Header" in " ".join([body[start]] + [x for x in body[start + 1:start + 8] if x.strip().startswith(";")])):
            start -= 1
        if c[0] - start > 6 * GAP or not any(re.match(r"\s*ds_read_b32 ", l) for l in body[start:c[0]]):
            continue
        end = c[-1]
        while end + 1 < len(body) and not re.match(r"^\.LBB\d+_\d+:|\s*s_cbranch|\s*s_branch", body[end + 1]):
            end += 1
        span = body[start:end + 2]
        if any(re.match(r"\s*ds_read_(u16|b128)", l) for l in span):
            continue                                        # the tile store's sampler (long rays)
        out.append((start, end + 1, sum(1 for l in span if re.match(r"\s*ds_read_b32 ", l))))
    return out


def main():
    asm, remarks = compile_asm()
    print("kernel figures (compiler remarks): %s" % "  ".join("%s: %s" % (k, v) for k, v in sorted(kernel_figures(remarks).items())))
    i = 0
    while i < len(asm):
        m = re.match(r"^(_Z\w+):", asm[i])
        if m and re.search(CALLEES, m.group(1)):
            end = next(k for k in range(i, len(asm)) if asm[k].startswith(".Lfunc_end"))
            body = asm[i:end]
            for start, stop, n in samplers(body):
                cnt = dict(valu=0, ds=0, waits=0, salu=0)
                for l in body[start:stop + 1]:
                    c = classify(l)
                    if c:
                        cnt[c] += 1
                per = {k: round(v * 16.0 / n, 1) for k, v in cnt.items()}
                print("%-44s lines %5d-%5d  %2d samples  per 16 samples: VALU %5.1f  DS %4.1f  s_waitcnt %4.1f  other SALU %4.1f   waits: %s" % (
                    m.group(1)[:44], start, stop, n, per["valu"], per["ds"], per["waits"], per["salu"],
                    " ".join(re.sub(r"\s+", "", l.split("s_waitcnt")[1]) for l in body[start:stop + 1] if l.strip().startswith("s_waitcnt"))))
            i = end
        i += 1


if __name__ == "__main__":
    main()
