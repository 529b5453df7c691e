"""Compare the device assembly of two builds kernel by kernel: same kernels, same instruction streams, same resources?
usage: python tools/asm_compare.py OLD.s NEW.s      (hipcc --cuda-device-only -S outputs, as tools/isa_count.py makes them)
One line per kernel: `same` / `DIFFERENT` with the VGPR, SGPR, scratch, LDS and accum_offset figures of both sides, then
the kernels only one side has.  Kernels are matched by demangled name; k_gradient's parameter list may differ between
the two files (the old <NCH = 1, TGV, LOG, J, NT, PX = 2> against <TGV, LOG, J, NT>).  Compared: every instruction with
its operands, after symbol names, local labels, comments and debug directives have been stripped.  For a kernel whose
stream differs the line also says how much of the difference is more than a renaming of registers.  Exit status 1 when
anything differs."""
import difflib
import re
import subprocess
import sys

FIGURES = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size", "accum_offset")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def canonical(name):
    """void j2p::k_gradient<1, true, false, 3, 0, 2>(j2p::GradArgs) -> the new parameter list <true, false, 3, 0>"""
    m = re.match(r"(.*\bk_gradient<)([^>]*)(>.*)", name)
    if m:
        args = [a.strip() for a in m.group(2).split(",")]
        if len(args) == 6 and args[0] == "1" and args[5] == "2":
            args = args[1:5]
        name = m.group(1) + ", ".join(args) + m.group(3)
    return name


def kernels(path):
    text = open(path).read()
    symbols = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    dem = demangle(symbols)
    found = {}
    for sym in symbols:
        begin = text.index("\n" + sym + ":")
        end = text.index(".end_amdhsa_kernel", begin)
        body, descriptor = text[begin:end].split(".amdhsa_kernel", 1)
        stream = []
        for line in body.split("\n")[2:]:
            line = line.split(";")[0].strip()
            if not line or line.endswith(":") or line.startswith("."):
                continue
            line = re.sub(r"\.L\w+", "L", line)                  # local labels (branch targets)
            for s in symbols:                                     # symbol names (none expected inside a kernel)
                line = line.replace(s, "SYM")
            stream.append(line)
        figures = {f: re.search(r"\.amdhsa_" + f + r"\s+(\S+)", descriptor).group(1) for f in FIGURES}
        found[canonical(dem[sym])] = (stream, figures)
    return found


def beyond_renaming(old, new):
    """instructions that have no counterpart on the other side even with register numbers ignored"""
    def blank(stream):
        return [re.sub(r"\b([sva])(\d+|\[\d+:\d+\])", r"\1N", line) for line in stream]
    ops = [op for op in difflib.SequenceMatcher(None, blank(old), blank(new), autojunk=False).get_opcodes() if op[0] != "equal"]
    return f"beyond register names: {sum(op[2] - op[1] for op in ops)} old / {sum(op[4] - op[3] for op in ops)} new"


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(set(old) & set(new)):
        (so, fo), (sn, fn) = old[name], new[name]
        same = so == sn and fo == fn
        bad += not same
        show = " ".join(f"{k} {fo[k]}" + ("" if fo[k] == fn[k] else f" -> {fn[k]}") for k in FIGURES)
        what = "same" if same else "DIFFERENT" + ("" if so == sn else f" (instructions {len(so)} -> {len(sn)}; {beyond_renaming(so, sn)})")
        print(f"{what:10s} {len(sn):6d} instructions  {show}  {name}")
    for name in sorted(set(old) - set(new)):
        bad += 1
        print(f"ONLY OLD   {name}")
    for name in sorted(set(new) - set(old)):
        bad += 1
        print(f"ONLY NEW   {name}")
    print(f"{len(set(old) & set(new))} kernels in both, {len(set(old) - set(new))} only old, {len(set(new) - set(old))} only new, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
