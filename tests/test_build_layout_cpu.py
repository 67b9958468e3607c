"""Which translation unit owns which kernels, read from the built library: the token step's kernels are instantiated in ONE unit
(csrc/t5.hip), and the decode host path (csrc/t5_generate.hip) has no device code at all -- so a change to the host path can
neither move nor recompile a kernel.  Structure only: kernel names, code objects and the host's registration symbols."""
from __future__ import annotations

import importlib.util
import os
import re
import subprocess

import pytest

from mapperatorinator_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ckr():
    spec = importlib.util.spec_from_file_location("ckr", os.path.join(ROOT, "tools", "check_kernel_resources.py"))
    ckr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ckr)
    return ckr


def _symbols(ckr, path):
    """-> [(type, name)] of an ELF file's symbol table, in table order"""
    txt = subprocess.run([os.path.join(ckr.LLVM, "llvm-readelf"), "--symbols", "--wide", path], check=True, capture_output=True,
                         text=True).stdout
    return [(f[3], f[7]) for f in (ln.split() for ln in txt.splitlines()) if len(f) >= 8 and f[0].rstrip(":").isdigit()]


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    """-> (unit_cuid, objects): unit_cuid {source file: the id of the device code it registers, None if it registers none} from the
    library's own symbol table (a unit's local symbols follow its FILE symbol; `__hip_gpubin_handle_<id>` is what hipcc gives a unit
    with device code); objects {id: demangled kernel names} per code object (its `__hip_cuid_<id>` symbol)"""
    ckr = _ckr()
    lib = _lib.lib_path()
    unit_cuid, cur = {}, None
    for typ, name in _symbols(ckr, lib):
        if typ == "FILE":
            cur = name
            if name.endswith(".hip"):
                unit_cuid[name] = None
        elif cur in unit_cuid and name.startswith("__hip_gpubin_handle_"):
            unit_cuid[cur] = name[len("__hip_gpubin_handle_"):]
    objects = {}
    td = tmp_path_factory.mktemp("co")
    for i, elf in enumerate(ckr.code_objects(lib)):
        co = td / f"{i}.co"
        co.write_bytes(elf)
        cuids = sorted({n[len("__hip_cuid_"):] for _, n in _symbols(ckr, str(co)) if n.startswith("__hip_cuid_")})   # (.dynsym and .symtab)
        assert len(cuids) == 1 and cuids[0] not in objects, cuids
        objects[cuids[0]] = ckr.demangle([k[".symbol"].removesuffix(".kd") for k in ckr.kernels_of(elf)])
    return unit_cuid, objects


def _kernel(nm: str) -> str:
    """the plain name of a demangled kernel: `void mh::dec::gemv_kernel<float, ...>(...)` -> gemv_kernel"""
    return re.split(r"[<(]", nm.removeprefix("void ").replace("(anonymous namespace)::", ""))[0].split("::")[-1]


def test_no_kernel_is_in_two_code_objects(layout):
    unit_cuid, objects = layout
    assert len(objects) >= 10 and sum(len(k) for k in objects.values()) > 600
    assert set(objects) <= {c for c in unit_cuid.values() if c}, "a code object that no unit of the library registers"
    seen = {}
    for cuid, names in objects.items():
        for nm in names:
            assert nm not in seen, f"{nm} is in the code objects {seen[nm]} and {cuid}"
            seen[nm] = cuid


def test_the_token_step_kernels_are_in_one_unit(layout):
    """every kernel named dec_*, and the GEMV / fused-tail kernels of decode_kernels.hpp, in the code object of t5.hip"""
    unit_cuid, objects = layout
    step = unit_cuid.get("t5.hip")
    assert step and step in objects, unit_cuid
    where, other = {}, set()
    for cuid, names in objects.items():
        for nm in names:
            k = _kernel(nm)
            if k.startswith("dec_") or "mh::dec::" in nm:     # a decode kernel by its name, or by the namespace of decode_kernels.hpp
                where.setdefault(k, set()).add(cuid)
            elif "dec_" in k:
                other.add(k)
    # the one other name that contains "dec_": the diffusion loop's step counter (dit.hip), no kernel of the decode
    assert other == {"loop_dec_kernel"}, other
    assert {"gemv_kernel", "dec_tail_kernel", "dec_self_attn_qkv_kernel", "dec_slot_self_attn_kernel", "dec_cross_attn_q_kernel",
            "dec_sample_kernel", "dec_init_kernel", "dec_slot_init_kernel", "dec_finalize_kernel"} <= set(where), sorted(where)
    assert all(v == {step} for v in where.values()), {k: v for k, v in where.items() if v != {step}}


def test_the_decode_host_path_has_no_device_code(layout):
    """t5_generate.hip is linked in (its FILE symbol) and registers no code object: no kernel can sit in that unit"""
    unit_cuid, objects = layout
    assert "t5_generate.hip" in unit_cuid and "t5.hip" in unit_cuid, sorted(unit_cuid)
    cuid = unit_cuid["t5_generate.hip"]
    assert cuid is None or not objects.get(cuid), objects.get(cuid)
