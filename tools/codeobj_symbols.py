"""Per-kernel comparison of two gfx950 device assembly files (the <file>-hip-amdgcn-amd-amdhsa-gfx950.s that hipcc --save-temps=obj
leaves; tools/compare_codeobj.sh --symbols builds both sides and calls this):
    python tools/codeobj_symbols.py BASE.s NEW.s
For every kernel of either file: 'identical' when the instruction text from its label to its kernel descriptor is equal (basic-block
labels carry the function's index in the file, which moves when an earlier instantiation goes: that index is masked), else 'DIFFERS',
or 'only in base' / 'only in new'; and the VGPR / AGPR / SGPR counts, LDS and scratch bytes of the metadata of both sides.  Exit
status 1 when a kernel present on both sides differs."""
import re
import sys


def bodies(path):
    out, name, lines = {}, None, []
    for line in open(path, encoding="utf-8", errors="replace"):
        m = re.match(r"^(\w+):\s+; @\1\s*$", line)
        if m:
            name, lines = m.group(1), []
        elif name and (line.startswith("\t.section\t.rodata") or line.startswith(".Lfunc_end")):      # (the kernel descriptor follows)
            out[name], name = "".join(lines), None
        elif name:
            line = line.split(";")[0].rstrip()       # (comments name source lines and value names)
            if line:
                lines.append(re.sub(r"\.L(BB|JTI)\d+_", r".L\1_", line) + "\n")
    return out


def metadata(path):
    text = open(path, encoding="utf-8", errors="replace").read().split("amdhsa.kernels:", 1)[1]
    out = {}
    for block in text.split("\n  - ")[1:]:
        f = dict(re.findall(r"^\s*\.(\w+):\s+(\S+)\s*$", block, flags=re.M))
        if "name" in f:
            out[f["name"]] = tuple(int(f.get(k, 0)) for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size",
                                                              "private_segment_fixed_size"))
    return out


def main():
    base, new = sys.argv[1], sys.argv[2]
    (fb, mb), (fn, mn) = (bodies(base), metadata(base)), (bodies(new), metadata(new))
    kernels = sorted(set(mb) | set(mn))
    rc = 0
    print("# kernel: verdict; vgpr agpr sgpr lds scratch (base -> new)")
    for k in kernels:
        if k not in mn:
            print(f"{k}: only in base; {mb[k]}")
        elif k not in mb:
            print(f"{k}: only in new; {mn[k]}")
        else:
            same = fb[k] == fn[k]
            rc |= 0 if same else 1
            print(f"{k}: {'identical' if same else 'DIFFERS'}; {mb[k]}" + ("" if mb[k] == mn[k] else f" -> {mn[k]}"))
    return rc


if __name__ == "__main__":
    sys.exit(main())
