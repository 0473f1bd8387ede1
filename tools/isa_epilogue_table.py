#!/usr/bin/env python3
"""Resources of the kernels in an assembly listing, one markdown row per kernel.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -S --cuda-device-only dcx_conv_h3.hip -o h3.s
    python tools/isa_epilogue_table.py h3.s [--match x3dw] [--other parent_h3.s]

Per kernel: code bytes, VGPRs, scratch bytes, the number of conditional branches, of scratch reloads
and of `s_waitcnt vmcnt(0)` in the whole body and after the main loop's last MFMA (the epilogue: the
static count over every path the form keeps, an upper bound of the executed ones).  With --other the
same columns of a second listing (the parent's) follow, matched by demangled kernel name.
"""
import argparse
import re
import subprocess


# EpiForm<epi, mean, y, y2, y6h, y6sh, track, rowwise> as dcx_conv_h3.hip names them
FORMS = {"0, 0, false, false, false, true, true, false": "EpiC1", "0, 0, true, false, false, true, true, false": "EpiUp",
         "3, 0, true, false, false, true, true, false": "EpiC2", "3, 1, false, false, false, false, false, false": "EpiMeanF",
         "3, 2, false, false, false, false, false, false": "EpiMeanM", "3, 3, false, false, false, true, true, false": "EpiMeanLH",
         "3, 3, false, true, false, false, true, false": "EpiMeanLF", "1, 0, false, false, true, false, false, true": "EpiPw1",
         "2, 0, true, false, false, false, false, false": "EpiPw2"}


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            body.append(line)
            if line.startswith(".Lfunc_end"):
                out[name] = {"body": body}
                name = None
    text = open(path).read()
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        if m.group(1) in out:
            v = re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2))
            s = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2))
            out[m.group(1)].update(vgpr=int(v.group(1)) if v else -1, scratch=int(s.group(1)) if s else -1)
    # "; codeLenInByte = N" follows each function's end label
    sizes = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.size\s+(_Z\w+), \.Lfunc_end.*?codeLenInByte = (\d+)", text, re.S)}
    for k, d in out.items():
        b = d.pop("body")
        code = [ln for ln in b if ln.startswith("\t") and not ln.startswith("\t.") and not ln.startswith("\t;")]
        last = max((i for i, ln in enumerate(code) if "v_mfma" in ln), default=-1)
        epi = code[last + 1:]
        d["bytes"] = sizes.get(k, -1)
        w0 = lambda ls: sum(1 for ln in ls if re.search(r"s_waitcnt.*vmcnt\(0\)", ln))  # noqa: E731
        d.update(branches=sum(1 for ln in code if "s_cbranch" in ln), reloads=sum(1 for ln in code if "scratch_load" in ln),
                 reloads_epi=sum(1 for ln in epi if "scratch_load" in ln), vm0=w0(code), vm0_epi=w0(epi), lines_epi=len(epi))
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    short = []
    for n in r:
        n = n.replace("void dcx::", "").replace("dcx::", "").replace("(dcx::ConvParams)", "").replace("(dcx::ConvGroup)", "")
        n = re.sub(r"\((ConvParams|ConvGroup)\)", "", n)
        n = n.replace("EpiGeneric", "generic")
        for args, form in FORMS.items():  # the forms by the names dcx_conv_h3.hip gives them
            n = n.replace(f"EpiForm<{args}> >", form + ">").replace(f"EpiForm<{args}>", form)
        short.append(n)
    return dict(zip(names, short))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("--match", default="")
    ap.add_argument("--other")
    a = ap.parse_args()
    cols = ("bytes", "vgpr", "scratch", "branches", "reloads", "reloads_epi", "vm0", "vm0_epi", "lines_epi")
    k = kernels(a.asm)
    names = demangle(list(k))
    other = {}
    if a.other:
        ko = kernels(a.other)
        other = {v: ko[n] for n, v in demangle(list(ko)).items()}
    print("| kernel | " + " | ".join(cols) + " |" + (" parent: " + " | ".join(cols) + " |" if a.other else ""))
    print("|---|" + "---|" * len(cols) * (2 if a.other else 1))
    for n in sorted(k, key=lambda z: names[z]):
        if a.match not in names[n]:
            continue
        row = f"| `{names[n]}` | " + " | ".join(str(k[n][c]) for c in cols) + " |"
        if a.other:
            o = other.get(names[n]) or other.get(names[n].replace(", generic", "")) or other.get(names[n].replace(", false, generic", ""))
            row += " " + (" | ".join(str(o[c]) for c in cols) if o else "-") + " |"
        print(row)


if __name__ == "__main__":
    main()
