"""Which translation unit owns which kernels, read from the built library: every decode kernel is instantiated in the ONE unit of its
family (csrc/decode_gemv.hip, decode_attn_bf16.hip / decode_attn_f32.hip, decode_sample.hip), and the decode host path
(csrc/t5_step.hip, t5_generate.hip) has no device code at all -- so a change to the host path can neither move nor recompile a kernel,
and a change to one family recompiles that family alone.  Structure only: kernel names, code objects and the host's registration
symbols."""
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


# The decode kernels and the unit that instantiates each.  A decode kernel: one whose name starts with `dec_`, or that lives in
# mh::dec, or the step-wise embed, or one of the three e4m3 quantisers.  The attention kernels are cut by storage type (their first
# template argument): every instantiation of one type is in that type's unit.
_ATTN = {"float": "decode_attn_f32.hip", "unsigned short": "decode_attn_bf16.hip"}
DECODE_KERNELS = {
    "gemv_kernel": "decode_gemv.hip", "dec_tail_kernel": "decode_gemv.hip",
    "dec_self_attn_qkv_kernel": _ATTN, "dec_slot_self_attn_kernel": _ATTN, "dec_cross_attn_q_kernel": _ATTN,
    "dec_sample_kernel": "decode_sample.hip", "dec_init_kernel": "decode_sample.hip", "dec_slot_init_kernel": "decode_sample.hip",
    "dec_finalize_kernel": "decode_sample.hip", "step_embed_kernel": "decode_sample.hip",
    "kv_quant_fp8_kernel": "decode_sample.hip", "kv_quant_fp8_row_kernel": "decode_sample.hip",
    "self_kv_quant_rows_kernel": "decode_sample.hip",
}
_QUANTISERS = {"kv_quant_fp8_kernel", "kv_quant_fp8_row_kernel", "self_kv_quant_rows_kernel"}


def test_every_decode_kernel_is_in_the_unit_of_its_family(layout):
    """every instantiation of a decode kernel is in exactly the code object that DECODE_KERNELS names for it, and the decode
    kernels are exactly the names of that table"""
    unit_cuid, objects = layout
    where, other = {}, set()
    for cuid, names in objects.items():
        for nm in names:
            k = _kernel(nm)
            if k.startswith("dec_") or "mh::dec::" in nm or k == "step_embed_kernel" or k in _QUANTISERS:
                first_arg = re.search(r"<([^,>]*)", nm)
                where.setdefault((k, first_arg.group(1) if first_arg else None), set()).add(cuid)
            elif "dec_" in k:
                other.add(k)
    # the one other name that contains "dec_": the diffusion loop's step counter (dit.hip), no kernel of the decode
    assert other == {"loop_dec_kernel"}, other
    assert {k for k, _ in where} == set(DECODE_KERNELS), sorted(where)
    wrong = {}
    for (k, t), cuids in where.items():
        unit = DECODE_KERNELS[k]
        if isinstance(unit, dict):
            assert t in unit, (k, t)
            unit = unit[t]
        assert unit_cuid.get(unit), (unit, unit_cuid)
        if cuids != {unit_cuid[unit]}:
            wrong[(k, t)] = cuids
    assert not wrong, wrong
    for k, unit in DECODE_KERNELS.items():     # an attention kernel has instantiations of both storage types, each in its unit
        if isinstance(unit, dict):
            assert {t for kk, t in where if kk == k} == set(unit), k
    # and the decode units hold nothing else
    for unit in {u for v in DECODE_KERNELS.values() for u in (v.values() if isinstance(v, dict) else [v])}:
        assert {_kernel(nm) for nm in objects[unit_cuid[unit]]} <= set(DECODE_KERNELS), unit


def test_the_decode_host_path_has_no_device_code(layout):
    """t5_generate.hip and t5_step.hip (enqueue_step, the operand descriptions) are linked in (their FILE symbols) and register no
    code object: no kernel can sit in those units"""
    unit_cuid, objects = layout
    assert "t5.hip" not in unit_cuid, sorted(unit_cuid)
    for unit in ("t5_generate.hip", "t5_step.hip"):
        assert unit in unit_cuid, sorted(unit_cuid)
        cuid = unit_cuid[unit]
        assert cuid is None or not objects.get(cuid), (unit, objects.get(cuid))
