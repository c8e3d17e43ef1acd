#!/usr/bin/env python3
"""Every s_waitcnt that names vmcnt in one kernel, by the FG_MARK() it follows (device assembly, -DFG_ASM_MARKS, the compile line of
tools/valu_count.py).

gfx950 counts loads AND stores on vmcnt and retires them in order, so a vmcnt wait inside the streaming loop (fg_pipeline.hpp) is a
wait for the next group's register window -- or for the row stores in front of it -- unless it stands where the window has landed
anyway (stage A).  The listing is by position in the assembly text: a wait belongs to the last mark printed before it, and it is
`rare` when it stands between a RARE_BEGIN and a RARE_END mark.  Blocks the compiler moved out of line keep their own marks, which is
what the brackets are for.  Position is all the listing knows: brackets that do not pair up in the text (an end laid out ahead of
its begin, a loop mark inside a bracket) are reported as warnings, and a listing with warnings proves nothing.

usage: tools/hot_waits.py flowgger_amd/csrc/fg_rfc5424.hip k_rfc5424ILi20ELb0ELb0ELb0E [--json] [-D...]
       HOT_WAITS_ASM=file.s reads an assembly file instead of compiling."""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assembly(src, extra):
    if os.environ.get("HOT_WAITS_ASM"):
        return open(os.environ["HOT_WAITS_ASM"]).read()
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "hot_waits.s")
        hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        cmd = [hipcc, "--offload-arch=gfx950", "-x", "hip", "-O3", "-std=c++17", "-fno-fast-math", "-ffp-contract=off",
               "-DFG_ASM_MARKS", f"-I{ROOT}/include", f"-I{ROOT}/tests/native", "--cuda-device-only", "-S", src, "-o", out] + extra
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
        return open(out).read()


def scan(s, pat):
    m = re.search(r"^(\S*%s[^\s:]*):.*\n" % re.escape(pat), s, re.M)
    if not m:
        sys.exit("kernel not found; candidates:\n" + "\n".join(re.findall(r"^(_Z[^\s:]+):.*$", s, re.M)))
    body = s[m.end():]
    end = body.find(".end_amdhsa_kernel")
    body = body[:end] if end >= 0 else body
    label, rare, n_ins = "(entry)", 0, 0
    marks, waits, warnings = [], [], []
    line0 = s.count("\n", 0, m.end()) + 1  # (line numbers of the assembly file, for looking a wait up)
    for i, ln in enumerate(body.split("\n")):
        t = ln.strip()
        if "FGMARK" in t:
            k = t.split("FGMARK")[1].strip()
            if k == "RARE_BEGIN":
                if rare:
                    warnings.append("RARE_BEGIN inside a rare block at instruction %d (behind %s)" % (n_ins, label))
                rare += 1
            elif k == "RARE_END":
                if not rare:  # (the compiler laid the block's end out ahead of its begin: the listing around it cannot be trusted)
                    warnings.append("RARE_END without a RARE_BEGIN at instruction %d (behind %s)" % (n_ins, label))
                rare = max(rare - 1, 0)
            else:
                if rare:
                    warnings.append("mark %s inside a rare block at instruction %d" % (k, n_ins))
                label = k
            marks.append({"mark": k, "at": n_ins})
            continue
        if not t or t[0] in ";." or t.endswith(":"):
            continue
        n_ins += 1
        if t.startswith("s_waitcnt"):
            w = re.search(r"vmcnt\((\d+)\)", t)
            if w:
                waits.append({"after": label, "rare": rare > 0, "vmcnt": int(w.group(1)), "at": n_ins, "line": line0 + i, "text": " ".join(t.split())})

    if rare:
        warnings.append("%d RARE_BEGIN without a RARE_END at the kernel's end" % rare)

    def figure(key):
        f = re.compile(r"^;\s*%s:\s*(\d+)" % key, re.M).search(s, m.end())  # (the resource comments follow the kernel's body)
        return int(f.group(1)) if f else None

    return {"kernel": m.group(1), "marks": marks, "waits": waits, "vgprs": figure("NumVgprs"), "scratch": figure("ScratchSize"),
            "instructions": n_ins, "warnings": warnings}


def main():
    args = [a for a in sys.argv[1:] if a != "--json"]
    if len(args) < 2:
        sys.exit(__doc__)
    r = scan(assembly(args[0], args[2:]), args[1])
    if "--json" in sys.argv[1:]:
        print(json.dumps(r))
        return
    print(r["kernel"])
    print("marks (instruction index): " + "  ".join("%s@%d" % (k["mark"], k["at"]) for k in r["marks"]))
    print("%-8s %-5s %8s %8s  %s" % ("after", "rare", "at", "line", "wait"))
    for w in r["waits"]:
        print("%-8s %-5s %8d %8d  %s" % (w["after"], "rare" if w["rare"] else "-", w["at"], w["line"], w["text"]))
    by = {}
    for w in r["waits"]:
        k = (w["after"], w["rare"])
        by[k] = by.get(k, 0) + 1
    print("vmcnt waits by region: " + "  ".join("%s%s=%d" % (a, "(rare)" if q else "", n) for (a, q), n in by.items()))
    print("NumVgprs %s  ScratchSize %s  instructions %d" % (r["vgprs"], r["scratch"], r["instructions"]))
    for w in r["warnings"]:
        print("WARNING: " + w + ": waits may carry the wrong label")


main()
