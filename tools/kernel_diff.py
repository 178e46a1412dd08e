#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of librovmpc.so: names, resource metadata and instruction text.  No GPU needed.

    python tools/kernel_diff.py old.so new.so [--llvm /opt/rocm/llvm/bin] [--arch gfx950]

From each library every offload bundle of the .hip_fatbin section is taken (a library linked from several objects holds one per
object), its code object for the target is unbundled, the kernel metadata is read from the AMDGPU note and the text section is
disassembled.  Per kernel the tool compares vgpr / sgpr / agpr counts, spill counts, LDS, scratch and kernarg size, and the
instruction text.  It prints one line per kernel that differs or is missing, duplicates within a library, and a summary; the
exit status is 0 only when nothing differs.

What is left out of the instruction text, and what that hides:
- addresses, encodings and the disassembler's branch-target comments;
- the literal of the s_add_u32 / s_addc_u32 pair behind s_getpc_b64, the distance to a table or function elsewhere in the code
  object: a kernel that came to address another table, or to call another non-inlined device function, compares equal;
- trailing "s_nop 0", "..." and s_code_end, the padding up to the next symbol: a real trailing s_nop goes with it.
Only the symbols named in amdhsa.kernels are walked: the body of a device function that is not a kernel is not compared.
A module compiled at run time (hiprtc) is not in the library and is not covered."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = (".vgpr_count", ".sgpr_count", ".agpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
          ".private_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size", ".wavefront_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_objects(lib, llvm, arch, tmp):
    tag = os.path.basename(lib) + "." + str(abs(hash(lib)))
    fat = os.path.join(tmp, tag + ".fatbin")
    run(os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, tag + ".copy"))
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    out = []
    for i, s in enumerate(starts):
        part = os.path.join(tmp, f"{tag}.{i}.bundle")
        with open(part, "wb") as f:
            f.write(data[s:starts[i + 1] if i + 1 < len(starts) else len(data)])
        co = os.path.join(tmp, f"{tag}.{i}.co")
        run(os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + part, "--output=" + co,
            "--targets=hipv4-amdgcn-amd-amdhsa--" + arch)
        if os.path.getsize(co):
            out.append(co)
    return out


def metadata(co, llvm):
    """{kernel name: {field: value}} from the AMDGPU metadata note."""
    kernels, cur, inside = {}, None, False
    for line in run(os.path.join(llvm, "llvm-readelf"), "--notes", co).splitlines():
        if line.startswith("amdhsa.kernels:"):
            inside = True
            continue
        if inside and line and not line.startswith(" "):
            inside = False
        if not inside:
            continue
        m = re.match(r"^  (- | {2})(\.\w+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
            kernels[id(cur)] = cur
        cur[m.group(2)] = m.group(3).strip()
    return {k[".name"]: {f: k.get(f, "") for f in FIELDS} for k in kernels.values()}


def disassembly(co, llvm):
    """{symbol: [instruction text]} of the text section; addresses, encodings and target comments dropped."""
    funcs, cur, pcrel = {}, None, 0
    for line in run(os.path.join(llvm, "llvm-objdump"), "-d", "--no-show-raw-insn", co).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        if cur is None or not line.startswith("\t") and not line.startswith(" "):
            continue
        text = re.sub(r"\s+", " ", line.split("//")[0].strip())
        if not text:
            continue
        # the pair that follows s_getpc_b64 adds the distance to a table or function elsewhere in the code object: an
        # address, which moves with the kernel's place in its code object
        if text.startswith("s_getpc_b64"):
            pcrel = 2
        elif pcrel and re.match(r"s_addc?_u32 s\d+, s\d+, (0x[0-9a-f]+|-?\d+)$", text):
            text = re.sub(r", [^,]+$", ", <pc-relative>", text)
            pcrel -= 1
        cur.append(text)
    for body in funcs.values():                     # padding up to the next symbol or the end of the section
        while body and body[-1] in ("s_nop 0", "...", "s_code_end"):
            body.pop()
    return funcs


def load(lib, llvm, arch, tmp):
    meta, text, dup = {}, {}, []
    cos = code_objects(lib, llvm, arch, tmp)
    for co in cos:
        m, d = metadata(co, llvm), disassembly(co, llvm)
        for name in m:
            if name in meta:
                dup.append(name)
            meta[name] = m[name]
            text[name] = d.get(name, [])
    return len(cos), meta, text, dup


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--llvm", default="/opt/rocm/llvm/bin")
    ap.add_argument("--arch", default="gfx950")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        n_old, meta_old, text_old, dup_old = load(args.old, args.llvm, args.arch, tmp)
        n_new, meta_new, text_new, dup_new = load(args.new, args.llvm, args.arch, tmp)
    bad = 0
    for which, dup in (("old", dup_old), ("new", dup_new)):
        for name in sorted(set(dup)):
            print(f"DUPLICATE in {which}: {name}")
            bad += 1
    for name in sorted(set(meta_old) - set(meta_new)):
        print(f"MISSING in new: {name}")
        bad += 1
    for name in sorted(set(meta_new) - set(meta_old)):
        print(f"ADDED in new: {name}")
        bad += 1
    n_insn = 0
    for name in sorted(set(meta_old) & set(meta_new)):
        why = [f"{f[1:]} {meta_old[name][f]} -> {meta_new[name][f]}" for f in FIELDS if meta_old[name][f] != meta_new[name][f]]
        a, b = text_old[name], text_new[name]
        n_insn += len(a)
        if not a or not b:
            why.append("no instruction text found")
        elif a != b:
            first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            why.append(f"instructions {len(a)} -> {len(b)}, first difference at #{first}: "
                       f"'{a[first] if first < len(a) else '<end>'}' -> '{b[first] if first < len(b) else '<end>'}'")
        if why:
            print(f"DIFFERS: {name}: " + "; ".join(why))
            bad += 1
    print(f"old: {len(meta_old)} kernels in {n_old} code object(s); new: {len(meta_new)} kernels in {n_new} code object(s); "
          f"{len(set(meta_old) & set(meta_new))} in both, {n_insn} instructions compared; {bad} difference(s)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
