#!/usr/bin/env python3
"""Device code of two builds of libkiss_hip.so, kernel by kernel: python tools/kernel_diff.py OLD.so NEW.so

Extracts the gfx950 code objects of both libraries (as tests/test_small_finish_resources.py does), disassembles every
kernel and matches the kernels by demangled name.  Every kernel is reported: `DIFFERS` with registers, scratch, LDS,
spills and code size of both builds if the instruction streams differ (addresses, encodings and symbol annotations
dropped), else by its name without the parameter list in the list of identical ones.  Kernels that only one build has
are listed at the end.  Exit status 1 if a kernel differs or the new build lacks one.  No GPU needed."""
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile
import textwrap

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.test_small_finish_resources import LLVM_BIN, _kernels  # noqa: E402

FIGURES = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size",
           "vgpr_spill_count", "sgpr_spill_count")


def _tool(name, *args):
    return subprocess.run([os.path.join(LLVM_BIN, name)] + list(args), check=True, capture_output=True, text=True,
                          timeout=900).stdout


def _streams(code_object):
    """{symbol: (instruction lines without address / encoding / symbol annotations, code bytes)}"""
    out, cur, first, last = {}, None, {}, {}
    for line in _tool("llvm-objdump", "-d", "--no-show-raw-insn", code_object).splitlines():
        m = re.match(r"^([0-9a-f]+) <(.+)>:$", line)
        if m:
            cur = m.group(2)
            out[cur] = []
            continue
        if cur is None or not line.startswith("\t"):
            continue
        m = re.match(r"^\t(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        text, addr = (m.group(1), int(m.group(2), 16)) if m else (line.strip(), None)
        text = re.sub(r"\s*<[^>]*>", "", text)
        if text == "...":  # (zero padding behind the last kernel of a code object)
            continue
        out[cur].append(re.sub(r"\s+", " ", text))
        if addr is not None:
            first.setdefault(cur, addr)
            last[cur] = addr
    return {s: (tuple(v), last.get(s, 0) - first.get(s, 0)) for s, v in out.items()}


def load(lib):
    """[(demangled name, figures, stream, code bytes up to the last instruction)] over every kernel of `lib`"""
    found = []
    with tempfile.TemporaryDirectory() as work:
        md = _kernels(lib, work)
        streams = {}
        for f in sorted(os.listdir(work)):
            if "gfx950" in f:
                streams.update(_streams(os.path.join(work, f)))
        names = sorted(md)
        filt = next((p for p in (os.path.join(LLVM_BIN, "llvm-cxxfilt"), shutil.which("llvm-cxxfilt"), shutil.which("c++filt"))
                     if p and os.path.exists(p)), None)
        assert filt, "no llvm-cxxfilt or c++filt to demangle the kernel names with"
        demangled = subprocess.run([filt], input="\n".join(names) + "\n", check=True, capture_output=True, text=True,
                                   timeout=300).stdout.splitlines()
        assert len(demangled) == len(names)
        for sym, nice in zip(names, demangled):
            stream, size = streams[sym]
            found.append((nice, {k: md[sym].get(k, "?") for k in FIGURES}, stream, size))
    return found


def _short(name):
    """a demangled kernel name without return type, anonymous namespace and parameter list"""
    name = name.replace("(anonymous namespace)::", "")
    depth = 0
    for i, c in enumerate(name):
        depth += (c == "<") - (c == ">")
        if c == "(" and depth == 0:
            name = name[:i]
            break
    return name[5:] if name.startswith("void ") else name


def main(old_lib, new_lib):
    old, new = collections.defaultdict(list), collections.defaultdict(list)
    for side, lib in ((old, old_lib), (new, new_lib)):
        for nice, fig, stream, size in load(lib):
            side[nice].append((stream, fig, size))
    same = differ = 0
    identical = []
    for name in sorted(set(old) & set(new)):
        a, b = sorted(old[name]), sorted(new[name])  # (a name that several units have: paired in stream order)
        if [x[0] for x in a] == [x[0] for x in b]:
            same += len(a)
            identical.append(_short(name) + ("  (x%d)" % len(a) if len(a) > 1 else ""))
            continue
        differ += 1
        print("DIFFERS  %s" % name)
        for tag, side in (("old", a), ("new", b)):
            for stream, fig, size in side:
                print("    %s: %s code_bytes=%d instructions=%d" % (tag, " ".join("%s=%s" % kv for kv in fig.items()), size,
                                                                    len(stream)))
    print("identical:")
    print(textwrap.fill(", ".join(identical), 124, initial_indent="  ", subsequent_indent="  ", break_long_words=False))
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    for name in only_old:
        print("ONLY OLD %s" % name)
    for name in only_new:
        print("ONLY NEW %s" % name)
    print("%d kernels identical, %d differ, %d only in the old build, %d only in the new build" %
          (same, differ, len(only_old), len(only_new)))
    return 1 if differ or only_old else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
