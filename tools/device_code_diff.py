#!/usr/bin/env python
"""Compares the gfx950 device code of two builds of libmapperhip.so: per code object (one per translation unit, in link order)
the bytes of `.text`, `.rodata` and `.note` (`.note` holds every kernel's kernarg layout, register, LDS and scratch counts) and
the set of kernel symbols.  A host-only change must leave all of them as they were; the one thing that may move is the
`__hip_cuid_<hash>` symbol, which hashes the source file.  This is how "compiles to the same instructions" is checked.

usage: device_code_diff.py OLD.so NEW.so      exit status 0: only __hip_cuid_* symbols differ, 1: anything else differs,
                                              3: a tool (llvm-objcopy / -readelf, PyYAML) is missing or failed
       device_code_diff.py --kernel FRAGMENT OLD.so NEW.so
                                              for a change that adds kernels or moves them between code objects: the function bytes
                                              and the resource metadata (registers, LDS, scratch, spills, kernarg size: META) of every
                                              kernel of OLD whose mangled name contains FRAGMENT against the same kernel of NEW, found
                                              in whichever code object holds it (0: all equal, 1: one differs or is gone; FRAGMENT ""
                                              compares every kernel)"""
from __future__ import annotations

import hashlib
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_kernel_resources import LLVM, code_objects, demangle, kernels_of  # noqa: E402

SECTIONS = (".text", ".rodata", ".note")
# what a kernel's `.note` record says of its resources (the record also names the kernel and types its arguments: a kernel whose
# parameter type moved to another namespace keeps all of these)
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count",
        ".sgpr_spill_count", ".kernarg_segment_size", ".kernarg_segment_align", ".max_flat_workgroup_size", ".wavefront_size")


def describe(elf: bytes):
    """-> ({section: bytes}, kernel symbols, __hip_cuid_* symbols) of one code object"""
    with tempfile.TemporaryDirectory() as td:
        co = os.path.join(td, "a.co")
        open(co, "wb").write(elf)
        secs = {}
        for name in SECTIONS:
            out = os.path.join(td, "sec.bin")
            if os.path.exists(out):
                os.remove(out)
            subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", f"--only-section={name}", co, out], check=True)
            secs[name] = open(out, "rb").read() if os.path.exists(out) else b""
        syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--symbols", "--wide", co], check=True, capture_output=True,
                              text=True).stdout.split()
    return secs, {k[".symbol"] for k in kernels_of(elf)}, {s for s in syms if s.startswith("__hip_cuid_")}


def kernel_texts(lib_path: str, fragment: str):
    """-> {instantiation: (the bytes of its function in .text, its META values)} for every kernel of the library whose mangled name
    contains `fragment`"""
    out, meta = {}, {}
    for elf in code_objects(lib_path):
        recs = {k[".symbol"].removesuffix(".kd"): k for k in kernels_of(elf) if fragment in k[".symbol"]}
        wanted = set(recs)
        if not wanted:
            continue
        for sym, k in recs.items():
            if sym in meta:
                raise RuntimeError(f"{lib_path}: kernel {sym} is in two code objects")
            meta[sym] = tuple(k.get(f) for f in META)
        with tempfile.TemporaryDirectory() as td:
            co, sec = os.path.join(td, "a.co"), os.path.join(td, "text.bin")
            open(co, "wb").write(elf)
            subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.text", co, sec], check=True)
            text = open(sec, "rb").read()
            run = lambda *a: subprocess.run([os.path.join(LLVM, "llvm-readelf"), *a, "--wide", co], check=True, capture_output=True,
                                            text=True).stdout
            base = next(int(f[f.index(".text") + 2], 16) for f in (ln.replace("[", " ").replace("]", " ").split()
                                                                    for ln in run("--sections").splitlines()) if ".text" in f)
            for ln in run("--symbols").splitlines():
                f = ln.split()
                if len(f) >= 8 and f[3] == "FUNC" and f[7] in wanted:
                    addr, size = int(f[1], 16), int(f[2], 0)
                    out[f[7]] = text[addr - base: addr - base + size]
    # keyed by the instantiation -- name and template arguments, without the parameter list: a dependent parameter type that is
    # spelled differently in the new source mangles differently although every old instantiation receives the same type
    def instantiation(nm: str) -> str:   # the demangled name up to the "(" that opens the (last, top-level) parameter list
        end, depth = nm.rfind(")"), 0
        for i in range(end, -1, -1):
            depth += (nm[i] == ")") - (nm[i] == "(")
            if depth == 0:
                return nm[:i]
        return nm
    syms = sorted(out)
    res = {instantiation(nm): (out[s], meta[s]) for s, nm in zip(syms, demangle(syms))}
    if len(res) != len(out):   # two kernels that differ in their parameters only, or one anonymous-namespace name in two units
        raise RuntimeError(f"{lib_path}: {len(out)} kernels have only {len(res)} distinct instantiation names")
    return res


def main_kernels(old_lib: str, new_lib: str, fragment: str) -> int:
    """--kernel FRAGMENT: a change that ADDS instantiations moves the code object as a whole; what must hold then is that every
    kernel the old build has comes out with the same instructions (branches are pc-relative, so equal code has equal bytes)"""
    return compare_kernels(kernel_texts(old_lib, fragment), kernel_texts(new_lib, fragment), fragment, old_lib)


def compare_kernels(old: dict, new: dict, fragment: str = "", old_lib: str = "the old build") -> int:
    """{instantiation: (function bytes, META values)} of two builds -> 0: every kernel of `old` is in `new` with the same bytes and
    metadata, 1: one differs or is gone"""
    if not old:
        raise RuntimeError(f"no kernel matching {fragment!r} in {old_lib}")
    # a change that adds a template flag (defaulted to false, at the end of the list) renames every old instantiation to
    # `<..., false>`: an old name that is gone is compared with the new name that only appends `false` arguments to it
    for s in sorted(old):
        if s in new or not s.endswith(">"):
            continue
        for n_flags in (1, 2, 3):
            renamed = s[:-1] + ", false" * n_flags + ">"
            if renamed in new:
                new[s] = new.pop(renamed)
                break
    changed = [s for s in sorted(old) if s in new and old[s] != new[s]]
    gone = [s for s in sorted(old) if s not in new]
    for s in changed:
        (ob, om), (nb, nm) = old[s], new[s]
        if ob != nb:
            print(f"!! {s}: {len(ob)} bytes {hashlib.sha1(ob).hexdigest()[:12]} -> {len(nb)} bytes {hashlib.sha1(nb).hexdigest()[:12]}")
        for f, a, b in zip(META, om, nm):
            if a != b:
                print(f"!! {s}: {f} {a} -> {b}")
    for s in gone:
        print(f"!! removed: {s}")
    print(f"{len(old)} kernels matching {fragment!r} in the old build: {len(old) - len(changed) - len(gone)} with identical bytes and metadata, "
          f"{len(changed)} changed, {len(gone)} removed; {len(set(new) - set(old))} added by the new build")
    return 1 if changed or gone else 0


def main(argv):
    if len(argv) == 4 and argv[0] == "--kernel":
        return main_kernels(argv[2], argv[3], argv[1])
    if len(argv) != 2:
        print(__doc__, file=sys.stderr)
        return 3
    old, new = (code_objects(p) for p in argv)
    if not old or not new:
        raise RuntimeError("no gfx950 code objects found in %s" % (argv[0] if not old else argv[1]))
    n_diff = n_cuid = 0
    if len(old) != len(new):
        print(f"!! {len(old)} code objects against {len(new)}")
        n_diff += 1
    for i, (a, b) in enumerate(zip(old, new)):
        (sa, ka, ca), (sb, kb, cb) = describe(a), describe(b)
        for name in SECTIONS:
            if sa[name] != sb[name]:
                n_diff += 1
                print(f"!! code object {i}: {name} differs ({len(sa[name])} bytes {hashlib.sha1(sa[name]).hexdigest()[:12]} -> "
                      f"{len(sb[name])} bytes {hashlib.sha1(sb[name]).hexdigest()[:12]})")
        for sym in sorted(ka ^ kb):
            n_diff += 1
            print(f"!! code object {i}: kernel {'removed' if sym in ka else 'added'}: {sym}")
        if ca != cb:
            n_cuid += 1
            print(f"   code object {i}: {' '.join(sorted(ca))} -> {' '.join(sorted(cb))}")
    print(f"{min(len(old), len(new))} code objects compared ({', '.join(SECTIONS)}, kernel symbols): "
          f"{'DIFFERENT in %d places' % n_diff if n_diff else 'identical'}; {n_cuid} with another __hip_cuid_ symbol")
    return 1 if n_diff else 0


if __name__ == "__main__":
    try:
        rc = main(sys.argv[1:])
    except Exception:
        import traceback
        traceback.print_exc()
        rc = 3
    sys.exit(rc)
