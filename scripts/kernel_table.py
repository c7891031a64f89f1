#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds from their device assembly, no GPU
needed.  For each unit of each build:

  hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude -Ikaldi-ctc_amd/csrc \\
        --cuda-device-only -S kaldi-ctc_amd/csrc/UNIT.hip -o UNIT.s

  scripts/kernel_table.py --before OLD.s [...] --after NEW.s [...]

One line per kernel: whether the instruction text of its body is the same
(comments dropped, local labels numbered in order of appearance), and VGPRs
(arch + acc), AGPRs, SGPRs, scratch bytes, LDS bytes and kernarg bytes from
the code object metadata, before -> after; then the device functions that
were not inlined.  Exit status 1 if a kernel exists in only one build, is
defined twice in a build, or a resource grew."""
import argparse
import re
import subprocess
import sys

FIELDS = ["vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size",
          "kernarg_segment_size"]


def parse(path, kernels, funcs):
    text = open(path).read()
    lines = text.split("\n")
    bodies, name, body = {}, None, []
    for ln in lines:
        if name is None:
            m = re.match(r"^([A-Za-z_][\w$.]*):", ln)
            if m and not m.group(1).startswith(".L"):
                name, body = m.group(1), []
            continue
        if re.match(r"^\.Lfunc_end\d+:", ln):
            bodies[name], name = body, None
            continue
        ln = ln.split(";")[0].strip()
        if ln:
            body.append(ln)
    meta = text[text.index(".amdgpu_metadata"):] if ".amdgpu_metadata" in text else ""
    for entry in re.split(r"\n  - (?=\.)", meta)[1:]:
        m = re.search(r"^\s*\.name:\s+(\S+)", entry, re.M)
        if not m:
            continue
        res = []
        for f in FIELDS:
            v = re.search(r"^\s*(?:- )?\.%s:\s+(\d+)" % f, "    " + entry, re.M)
            res.append(int(v.group(1)) if v else 0)
        if m.group(1) in kernels:
            raise SystemExit(f"{m.group(1)} is defined in two units ({path})")
        kernels[m.group(1)] = (normalise(bodies.pop(m.group(1))), res)
    for n, b in bodies.items():  # device functions the kernels call
        funcs.setdefault(n, []).append(normalise(b))


def normalise(body):
    ids = {}

    def num(m):
        return ids.setdefault(m.group(0), f"L{len(ids)}")
    return [re.sub(r"\.L\w+", num, ln) for ln in body]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--before", nargs="+", required=True)
    ap.add_argument("--after", nargs="+", required=True)
    a = ap.parse_args()
    old, new, fold, fnew = {}, {}, {}, {}
    for f in a.before:
        parse(f, old, fold)
    for f in a.after:
        parse(f, new, fnew)
    names = sorted(set(old) | set(new))
    pretty = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")
    bad = 0
    print(f"# kernels: {len(old)} before, {len(new)} after; columns: text, vgpr agpr sgpr scratch lds kernarg")
    for n, p in zip(names, pretty):
        p = p.replace("kctc::(anonymous namespace)::", "").replace("void ", "")
        if n not in old or n not in new:
            print(f"{p}: only {'before' if n in old else 'after'}")
            bad = 1
            continue
        same = old[n][0] == new[n][0]
        ro, rn = old[n][1], new[n][1]
        grew = any(y > x for x, y in zip(ro, rn))
        bad |= grew
        res = " ".join(map(str, ro)) if ro == rn else " ".join(map(str, ro)) + " -> " + " ".join(map(str, rn))
        print(f"{p}: {'IDENTICAL' if same else f'differs ({len(old[n][0])} -> {len(new[n][0])} lines)'}  {res}"
              + ("  GREW" if grew else ""))
    for n in sorted(set(fold) | set(fnew)):
        same = fold.get(n) is not None and fnew.get(n) is not None and all(b == fold[n][0] for b in fold[n] + fnew[n])
        lines = [" ".join(str(len(b)) for b in f.get(n, [])) or "-" for f in (fold, fnew)]
        print(f"device function {n}: {'IDENTICAL' if same else 'differs'} ({lines[0]} -> {lines[1]} lines, "
              "one count per unit that keeps a copy)")
    return bad


if __name__ == "__main__":
    sys.exit(main())
