#!/usr/bin/env python3
"""Compare two assembly listings of one translation unit function by function.

    python tools/isa_diff.py OLD.s NEW.s [--resources OLD.txt NEW.txt] [--rename OLDSYM=NEWSYM ...]

OLD.s / NEW.s: hipcc <the flags of build_ext.py> --cuda-device-only -S (or --cuda-host-only -S).  A function is the text from
its `.type NAME,@function` to its `.Lfunc_end`, plus its `.amdhsa_kernel NAME` block.  Prints one line per file pair and the
names that differ or exist on one side only.  --resources: the stderr of -Rpass-analysis=kernel-resource-usage of both builds;
the resource lines of every differing kernel are printed side by side.  --rename: a kernel that changed its symbol (a template argument
more, another name) is compared under its new one -- every occurrence of OLDSYM in OLD.s and OLD.txt is read as NEWSYM.
"""
import re
import sys


RENAMES = []


def lines(path):
    for line in open(path):
        for old, new in RENAMES:
            line = line.replace(old, new)
        yield line


def functions(path, renamed=False):
    out, name, kern = {}, None, None
    for line in (lines(path) if renamed else open(path)):
        m = re.match(r"\s*\.type\s+([^,\s]+),@function", line)
        if m:
            name = m.group(1)
            out[name] = []
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            kern = m.group(1)
        if kern is not None:
            out.setdefault(kern, []).append(line)
            if ".end_amdhsa_kernel" in line:
                kern = None
        elif name is not None:
            out[name].append(line)
            if re.match(r"\s*\.Lfunc_end\d+:", line):
                name = None
    # local labels carry the function's ordinal in the file (it shifts when a function in front goes); host side: the fat binary's
    # symbols carry a hash of the source text
    def norm(text):
        text = re.sub(r"(?<!\w)((?:\.L)?BB|\.Lfunc_begin|\.Lfunc_end|\.LJTI|\.LCPI)\d+", r"\1", text)
        return re.sub(r"(__hip_(?:gpubin_handle|fatbin|cuid)_)[0-9a-f]+", r"\1ID", text)
    return {k: norm("".join(v)) for k, v in out.items()}


def resources(path, renamed=False):
    out, name = {}, None
    for line in (lines(path) if renamed else open(path)):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = []
        m = re.search(r"remark:\s+((?:VGPRs|AGPRs|ScratchSize|Occupancy|LDS Size|SGPRs Spill|VGPRs Spill)[^:]*: \d+)", line)
        if m and name:
            out[name].append(m.group(1).strip())
    return {k: ", ".join(v) for k, v in out.items()}


def main():
    while "--rename" in sys.argv:
        i = sys.argv.index("--rename")
        RENAMES.append(tuple(sys.argv[i + 1].split("=", 1)))
        del sys.argv[i:i + 2]
    old, new = functions(sys.argv[1], renamed=True), functions(sys.argv[2])
    res = [resources(sys.argv[4], renamed=True), resources(sys.argv[5])] if "--resources" in sys.argv else None
    both = sorted(set(old) & set(new))
    differ = [k for k in both if old[k] != new[k]]
    print("%s: %d functions before, %d after, %d on both sides, %d identical, %d differ, %d removed, %d added"
          % (sys.argv[2], len(old), len(new), len(both), len(both) - len(differ), len(differ), len(set(old) - set(new)), len(set(new) - set(old))))
    for k in differ:
        print("  differs: %s" % k)
        if res:
            print("    before: %s\n    after:  %s" % (res[0].get(k, "-"), res[1].get(k, "-")))
    for k in sorted(set(old) - set(new)):
        print("  removed: %s" % k)
    for k in sorted(set(new) - set(old)):
        print("  added:   %s" % k)
    return 1 if differ or set(new) - set(old) else 0


if __name__ == "__main__":
    sys.exit(main())
