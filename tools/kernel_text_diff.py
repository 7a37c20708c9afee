"""Which kernels of a translation unit changed?  Compares two device assembly listings of the same .hip file, kernel by kernel:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S csrc/attn.hip -o before.s     (on the parent commit)
    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S csrc/attn.hip -o after.s
    python tools/kernel_text_diff.py before.s after.s

A kernel is the text between its label and its .Lfunc_end; basic-block labels carry the function's ordinal in the file
(.LBB<ordinal>_<block>), which moves when a kernel is added in front, so the ordinal is dropped before comparing.  Prints one line
per kernel: identical / DIFFERS / NEW / GONE, and exits 1 if any kernel present in both listings differs."""
import re
import sys


def kernels(path):
    out, name, buf = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, buf = m.group(1), []
        elif name is not None:
            if re.match(r"^\.Lfunc_end\d+:", line):
                out[name], name = re.sub(r"\.LBB\d+_", ".LBB_", "".join(buf)), None
            else:
                buf.append(re.sub(r"\s*;.*$", "", line))  # comments name blocks by the same ordinal
    return out


def main(before, after):
    b, a = kernels(before), kernels(after)
    bad = 0
    for k in a:
        if k not in b:
            print("NEW      ", k, a[k].count("\n"), "lines")
        elif a[k] != b[k]:
            print("DIFFERS  ", k)
            bad = 1
        else:
            print("identical", k, a[k].count("\n"), "lines")
    for k in b:
        if k not in a:
            print("GONE     ", k)
    return bad


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
