"""Are the kernels of two builds the same instruction streams?
usage: python tools/isa_identity.py [--max-name N] [--alias OLD=NEW]... DIR_A DIR_B   (directories of `hipcc <build.py HIP_FLAGS> --offload-device-only -S` output, *.s)
Each kernel is keyed by its demangled name without the `(anonymous namespace)::` qualifier; its text (label to end marker,
comments dropped, local labels renamed by order of appearance) and its .amdhsa_ descriptor block are hashed together.
Prints one line per kernel with the hash of each side and a final count; exits 1 unless both sides hold the same kernels
with equal hashes.  --max-name N prints a name longer than N characters (hipCUB's template instances run to 2,800) as its
first N characters, `...` and the hash of the whole name: the comparison is still by whole names.  --alias OLD=NEW is for a
kernel that was renamed: DIR_A's kernel whose function name (the demangled name up to its parameter list, without `void `)
is OLD is keyed under the name of DIR_B's kernel whose function name is NEW, and its line says so."""
import glob
import hashlib
import os
import re
import subprocess
import sys


def kernels(directory):
    """{demangled name: [text, descriptor]} over every .s file of the directory"""
    found = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        with open(path) as f:
            lines = f.read().split("\n")
        start = {}
        for i, line in enumerate(lines):
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
            if m:
                end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
                found[m.group(1)] = [None, "\n".join(s.strip() for s in lines[i + 1:end])]
            m = re.match(r"(\w+):\s*(;.*)?$", line)
            if m:
                start[m.group(1)] = i
        for name, rec in found.items():
            if rec[0] is not None or name not in start:
                continue
            body, labels = [], {}
            for line in lines[start[name] + 1:]:
                if re.match(r"\.Lfunc_end\d+:", line):
                    break
                line = re.sub(r"\s*;.*$", "", line)  # (comments: whole lines and the notes after labels and instructions)
                if not line.strip():
                    continue
                line = line.replace(name, "<kernel>")
                body.append(re.sub(r"\.L[A-Za-z_]+\d+(_\d+)?", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), line))
            rec[0] = "\n".join(body)
    names = sorted(found)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for name, d in zip(names, plain):
        key = d.replace("(anonymous namespace)::", "")
        assert key not in out and found[name][0], key
        out[key] = found[name]
    return out


def digest(rec):
    return hashlib.sha256("\0".join(rec).encode()).hexdigest()[:16] if rec else "-"


def short(key, limit):
    if not limit or len(key) <= limit:
        return key
    return "%s...#%s" % (key[:limit], hashlib.sha256(key.encode()).hexdigest()[:12])


def function_name(key):
    return re.sub(r"^void ", "", key.split("(")[0])


def main():
    args, limit, aliases = sys.argv[1:], 0, []
    while args and args[0] in ("--max-name", "--alias"):
        if args[0] == "--max-name":
            limit = int(args[1])
        else:
            aliases.append(args[1].split("=", 1))
        args = args[2:]
    a, b = kernels(args[0]), kernels(args[1])
    was = {}
    for old, new in aliases:
        (ka,), (kb,) = [k for k in a if function_name(k) == old], [k for k in b if function_name(k) == new]
        assert kb not in a, kb
        a[kb] = a.pop(ka)
        was[kb] = old
    same = 0
    for key in sorted(set(a) | set(b)):
        ok = key in a and a[key] == b.get(key)
        same += ok
        note = "   (was %s)" % was[key] if key in was else ""
        print("%-9s %-16s %-16s %s%s" % ("same" if ok else "DIFFERENT", digest(a.get(key)), digest(b.get(key)), short(key, limit), note))
    name = [os.path.basename(os.path.normpath(d)) for d in args[:2]]
    print("%d kernels in %s, %d in %s, %d identical" % (len(a), name[0], len(b), name[1], same))
    return 0 if same == len(a) == len(b) else 1


if __name__ == "__main__":
    sys.exit(main())
