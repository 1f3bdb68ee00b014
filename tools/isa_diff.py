#!/usr/bin/env python3
"""Compare the gfx950 assembly of two builds, kernel by kernel (no GPU, no compiler).

    make BUILD=<a>/b LIBDIR=<a>/lib EXTRA_HIPFLAGS=-save-temps=obj      (in both trees)
    python tools/isa_diff.py <a>/b <b>/b

Pairs the *-hip-amdgcn-amd-amdhsa-gfx950.s files of the two build directories by name, drops what a
source-only change may alter (comments, .ident, .file, .loc, the __hip_cuid_<hash> symbol), splits each
listing per function symbol (code, .amdhsa_kernel block, metadata counts) and prints `identical` per
kernel, or the first differing lines and both sides' register / scratch counts. Exit status 1 on any
difference. Text comparison only: it knows nothing about particular instructions.
"""
import glob
import os
import re
import sys

SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"
COUNTS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count")
SHOW = 6  # differing lines printed per kernel


def normalise(text):
    out = []
    for line in text.splitlines():
        line = line.split(";", 1)[0].strip()
        if not line or line.split()[0] in (".ident", ".file", ".loc") or "__hip_cuid_" in line:
            continue
        # local labels carry the function's position in the file (.LBB<n>_<m>): only the order of instantiation
        out.append(re.sub(r"\.L(BB|func_begin|func_end)\d+", r".L\1", " ".join(line.split())))
    return out


def split_kernels(text):
    """{symbol: normalised lines}; '(file scope)' holds whatever belongs to no function."""
    code, _, meta = text.partition(".amdgpu_metadata")
    lines = normalise(code)
    funcs = {m.group(1) for l in lines if (m := re.match(r"\.type (\S+),@function$", l))}
    parts, cur = {"(file scope)": []}, "(file scope)"
    for l in lines:
        if (m := re.match(r"\.set ([^.\s]+)\.", l)) and m.group(1) in funcs:  # .set <symbol>.num_vgpr, ...
            parts.setdefault(m.group(1), []).append(l)
            continue
        if cur == "(file scope)":  # a function's part starts at the first line that names its symbol
            cur = next((t for t in re.split(r"[\s,:]+", l) if t in funcs), cur)
            if cur == "(file scope)" and l.split()[0] in (".text", ".section", ".p2align"):
                continue  # section switches between functions say nothing by themselves
        parts.setdefault(cur, []).append(l)
        if l.startswith((".size", ".end_amdhsa_kernel")):
            cur = "(file scope)"
    for item in re.split(r"(?m)^  - ", meta)[1:]:  # the metadata's kernel list: scalar keys of each kernel
        kv = re.findall(r"(?m)^(?:    )?(\.\w+):[ \t]+(\S+)[ \t]*$", item)
        if (name := dict(kv).get(".name")) is not None:
            parts.setdefault(name, []).extend(f"{k}: {v}" for k, v in kv if "__hip_cuid_" not in v)
    return parts


def counts(lines):
    return " ".join(l.replace(" ", "") for l in lines if l.split(":")[0] in COUNTS) or "(no metadata)"


def diff_listings(name, a, b, out=print):
    """Compare two listings; one line per kernel through `out`. Returns the number of differing kernels."""
    ka, kb, bad = split_kernels(a), split_kernels(b), 0
    for k in sorted(set(ka) | set(kb)):
        if k not in ka or k not in kb:
            out(f"{name}: {k}: only in {'first' if k in ka else 'second'}")
        elif ka[k] == kb[k]:
            out(f"{name}: {k}: identical")
            continue
        else:
            la, lb = ka[k], kb[k]
            out(f"{name}: {k}: DIFFERENT ({len(la)} / {len(lb)} lines)")
            i = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            for x, y in zip(la[i:i + SHOW] + [""] * SHOW, (lb[i:i + SHOW] + [""] * SHOW)[:SHOW]):
                out(f"    line {i}: {x!r} | {y!r}")
                i += 1
            out(f"    first:  {counts(la)}\n    second: {counts(lb)}")
        bad += 1
    return bad


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    fa, fb = ({os.path.basename(p)[:-len(SUFFIX)]: p for p in glob.glob(os.path.join(d, "*" + SUFFIX))} for d in argv[1:])
    bad = total = 0
    for tu in sorted(set(fa) | set(fb)):
        if tu not in fa or tu not in fb:
            print(f"{tu}: listing only in {'first' if tu in fa else 'second'}")
            bad += 1
            continue
        n = diff_listings(tu, open(fa[tu]).read(), open(fb[tu]).read())
        bad, total = bad + n, total + 1
    print(f"{total} listings compared, {bad} differences")
    return 1 if bad or not total else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
