#!/usr/bin/env python
"""Compares the gfx950 device code of two builds of libmapperhip.so: per code object (one per translation unit, in link order)
the bytes of `.text`, `.rodata` and `.note` (`.note` holds every kernel's kernarg layout, register, LDS and scratch counts) and
the set of kernel symbols.  A host-only change must leave all of them as they were; the one thing that may move is the
`__hip_cuid_<hash>` symbol, which hashes the source file.  This is how "compiles to the same instructions" is checked.

usage: device_code_diff.py OLD.so NEW.so      exit status 0: only __hip_cuid_* symbols differ, 1: anything else differs,
                                              3: a tool (llvm-objcopy / -readelf, PyYAML) is missing or failed"""
from __future__ import annotations

import hashlib
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_kernel_resources import LLVM, code_objects, kernels_of  # noqa: E402

SECTIONS = (".text", ".rodata", ".note")


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


def main(argv):
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
