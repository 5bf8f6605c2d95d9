#!/usr/bin/env python3
"""Did a change move code without changing a kernel?  Compares the device assembly of two builds kernel by kernel.

    hipcc <the Makefile's HIPFLAGS> -x hip --cuda-device-only -S FILE.hip -o FILE.s       (once per translation unit, old and new tree)
    scripts/kernel_asm_diff.py --old old/er_icp.s --new new/er_cloud.s new/er_icp.s new/er_ransac.s new/er_fpfh.s [--library-in er_cloud]

Kernels are matched by their demangled name with template arguments and parameter types, namespaces dropped (a kernel may move between an
anonymous namespace and a named one).  For every kernel that is not a library's (rocprim / hipcub) the instruction text must be the same --
comments and assembler directives dropped, local labels renumbered in order of appearance -- and so must .vgpr_count, .sgpr_count,
.group_segment_fixed_size and .private_segment_fixed_size of its metadata.  The set of library kernels must be the same on both sides and,
with --library-in STEM, every one of them defined only in the new file of that stem.  Prints one table row per kernel, a figure that moved as
"old -> new"; exit status 1 on any difference.

A change that edits a kernel's parameter list changes its signature, and the kernel would show as "only in the old build" and "only in the new
build".  --by-name pairs kernels by name and template arguments alone, so such a change reports as one row per kernel."""
import argparse
import os
import re
import subprocess
import sys

META = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")
LIBRARY = re.compile(r"\b(rocprim|hipcub)::")
CXXFILT = next((p for p in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "/usr/bin/c++filt") if os.path.exists(p)), "c++filt")


def demangle(names):
    names = list(names)
    if not names:
        return {}
    out = subprocess.run([CXXFILT], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def drop_namespaces(sig):
    """'void (anonymous namespace)::k<8>(er::Grid)' -> 'void k<8>(Grid)' (library names keep theirs: they are compared as a set only)."""
    if LIBRARY.search(sig):
        return sig
    return re.sub(r"(\(anonymous namespace\)|\b[A-Za-z_]\w*)::", "", sig)


def parse(path):
    """-> {mangled kernel symbol: (instruction lines, {metadata field: value})}"""
    lines = open(path).read().split("\n")
    kernels = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m]
    body, cur = {}, None
    for l in lines:
        s = l.split(";")[0].strip()
        if cur is None:
            if s.endswith(":") and s[:-1] in kernels and s[:-1] not in body:
                cur = s[:-1]
                body[cur] = []
            continue
        if re.match(r"\.Lfunc_end\d+:", s):
            cur = None
            continue
        if not s or (s.startswith(".") and not s.endswith(":")):
            continue
        body[cur].append(s)
    # the metadata note: "amdhsa.kernels:" at column 0, one "  - " list element per kernel with its own keys at column 4 (arguments sit deeper)
    meta, entry, inside = {}, {}, False
    for l in lines + ["end:"]:
        if l.startswith("amdhsa.kernels:"):
            inside = True
            continue
        if not inside or not l.strip():
            continue
        if l[0] != " " or l.startswith("  - "):
            if entry.get(".name") in body:
                meta[entry[".name"]] = {k: entry.get(k) for k in META}
            entry = {}
            if l[0] != " ":
                inside = False
                continue
        m = re.match(r"  [ -] (\.\w+):\s*(\S*)", l)
        if m:
            entry[m.group(1)] = m.group(2).strip("'")
    return {k: (body[k], meta.get(k, {})) for k in body}


def normalise(text, names):
    """Local labels renumbered in order of appearance; mangled symbols replaced by their namespace-free demangled form."""
    labels = {}

    def lab(m):
        return labels.setdefault(m.group(0), ".L%d" % len(labels))

    out = []
    for l in text:
        l = re.sub(r"\.L\w+", lab, l)
        l = re.sub(r"_Z\w+", lambda m: "<" + names.get(m.group(0), m.group(0)) + ">", l)
        out.append(re.sub(r"\s+", " ", l))
    return out


def load(paths, by_name=False):
    """-> {normalised signature: (file stem, instruction lines, metadata)}, {library signature: set of file stems}"""
    own, lib = {}, {}
    for p in paths:
        stem = os.path.splitext(os.path.basename(p))[0]
        k = parse(p)
        syms = set(k)
        for text, _ in k.values():
            for l in text:
                syms.update(re.findall(r"_Z\w+", l))
        names = {s: drop_namespaces(d) for s, d in demangle(sorted(syms)).items()}
        for sym, (text, meta) in k.items():
            sig = names[sym]
            if LIBRARY.search(sig):
                lib.setdefault(sig, set()).add(stem)
                continue
            if by_name:
                sig = short(sig)
            if sig in own:
                sys.exit("kernel defined twice: %s (%s, %s)" % (sig, own[sig][0], stem))
            own[sig] = (stem, normalise(text, names), meta)
    return own, lib


def short(sig):
    m = re.match(r"(?:void )?(.*?)\((?:[^()]|\([^()]*\))*\)$", sig)
    return m.group(1) if m else sig


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--library-in", default=None, help="stem of the one new file that may define rocprim / hipcub kernels")
    ap.add_argument("--by-name", action="store_true",
                    help="pair kernels by name and template arguments alone: for a change that edits parameter lists (two kernels of one name then count as defined twice)")
    a = ap.parse_args()
    old, old_lib = load(a.old, a.by_name)
    new, new_lib = load(a.new, a.by_name)
    if not old or not new:
        sys.exit("no kernels found in the %s files" % ("old" if not old else "new"))
    bad = 0
    print("| kernel | file | instructions | vgpr | sgpr | lds | scratch | verdict |")
    print("|---|---|---|---|---|---|---|---|")
    for sig in sorted(set(old) | set(new), key=short):
        o, n = old.get(sig), new.get(sig)
        if o is None or n is None:
            verdict = "only in the %s build" % ("new" if o is None else "old")
        else:
            what = []
            if o[1] != n[1]:
                first = next((i for i, (x, y) in enumerate(zip(o[1], n[1])) if x != y), min(len(o[1]), len(n[1])))
                what.append("text differs at instruction %d" % first)
            what += ["%s %s -> %s" % (f, o[2].get(f), n[2].get(f)) for f in META if o[2].get(f) != n[2].get(f) or o[2].get(f) is None]
            verdict = "; ".join(what) or "identical"
        bad += verdict != "identical"
        k = n or o

        def cell(get):                                            # "old -> new" where both builds have the kernel and the figure moved
            vals = [get(x) for x in (o, n) if x is not None]
            return str(vals[0]) if len(set(vals)) == 1 else "%s -> %s" % tuple(vals)

        cells = [cell(lambda x: sum(1 for l in x[1] if not l.endswith(":")))] + [cell(lambda x, f=f: x[2].get(f)) for f in META]
        print("| %s | %s | %s | %s |" % (short(sig), k[0], " | ".join(cells), verdict))
    print()
    print("%d kernels compared, %d not identical" % (len(set(old) | set(new)), bad))
    if set(old_lib) != set(new_lib):
        bad += 1
        for s in sorted(set(old_lib) - set(new_lib)):
            print("library kernel only in the old build:", s)
        for s in sorted(set(new_lib) - set(old_lib)):
            print("library kernel only in the new build:", s)
    else:
        print("%d library kernels (rocprim / hipcub): the same set in both builds" % len(new_lib))
    if a.library_in:
        stray = {s: f for s, f in new_lib.items() if f != {a.library_in}}
        bad += bool(stray)
        for s, f in sorted(stray.items()):
            print("library kernel defined in %s: %s" % (", ".join(sorted(f)), s))
        if not stray:
            print("every library kernel of the new build is defined in %s only" % a.library_in)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
