#!/usr/bin/env python3
"""Compare two device assembly files (hipcc --cuda-device-only -S) function by function.

usage: isa_diff.py OLD.s NEW.s

Prints one line per function: "same", or the two line counts when the text differs.  A function
is the text between its `.type NAME,@function` and `.size NAME` directives plus, for a kernel,
its `.amdhsa_kernel` descriptor; what lies outside every function (metadata, constants) is
compared as "(rest)".  Ignored: `;` comments, blank lines, the `__hip_cuid_*` symbol, and the
per-function index inside local labels (.LBB12_3 and .LBB13_3 compare equal).  Exit status 1
when anything differs.  The tool compares and does nothing else.
"""
import re
import sys

_TYPE = re.compile(r"\.type\s+([\w$.]+),@function")
_SIZE = re.compile(r"\.size\s+([\w$.]+),")
_DESC = re.compile(r"\.amdhsa_kernel\s+([\w$.]+)")
_LOCAL = re.compile(r"\.L(BB|func_begin|func_end|JTI|tmp)\d+")


def functions(path):
    """name -> list of normalised lines, in file order; "(rest)" collects the remainder."""
    out = {"(rest)": []}
    cur = None
    with open(path, errors="replace") as fh:
        for raw in fh:
            line = raw.split(";", 1)[0].strip()
            if not line or "__hip_cuid_" in line:
                continue
            line = _LOCAL.sub(lambda m: ".L" + m.group(1), line)
            m = _TYPE.match(line) or _DESC.match(line)
            if m:
                cur = m.group(1)
                out.setdefault(cur, [])
            out[cur if cur else "(rest)"].append(line)
            m = _SIZE.match(line)
            if (m and m.group(1) == cur) or line == ".end_amdhsa_kernel":
                cur = None
    return out


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    old, new = functions(argv[1]), functions(argv[2])
    differ = 0
    for name in list(old) + [n for n in new if n not in old]:
        a, b = old.get(name), new.get(name)
        if a == b:
            print(f"same       {name}")
        else:
            differ += 1
            na = "absent" if a is None else str(len(a))
            nb = "absent" if b is None else str(len(b))
            print(f"{na:>6} -> {nb:<6} {name}")
    print(f"{differ} of {len(set(old) | set(new))} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
