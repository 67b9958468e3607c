"""not gpu: which kernel mh_beam_step runs for a shape (mh_beam_step_path, option "beam_step_path") and what it still refuses.

The LDS kernel keeps its ground: K <= 4096 and 4 num_beams V (rounded up to 16) + 8 K' bytes (K' = K rounded up to a power of two)
within 120 KB = 122 880 B; everything else inside 2 .. 8 beams and K <= 8192 goes to the streaming kernel.  At K = 16 that line is
32 V + 128 <= 122 880, i.e. V <= 3836: (8, 3836, 16) is the last LDS shape and (8, 3837, 16) -- eight beams at the released
vocabulary -- the first streaming one.  (The issue that asked for these tests also listed (8, 3839, 16) as an LDS shape; 8 x 3839 x 4
= 122 848 B of scores + 128 B of candidates do not fit, and no rule can answer LDS there and streaming at V = 3837.  It is asserted
as the streaming shape it is, and the two shapes next to the line are asserted in its place.)"""
import ctypes as C
import os
import re
import types

import pytest

from conftest import ROOT
from mapperatorinator_amd import _lib


@pytest.fixture
def lib():
    lib = _lib.load()
    old = lib.mh_get_option(b"beam_step_path")
    yield lib
    assert lib.mh_set_option(b"beam_step_path", old) == 0


def test_beam_step_path_is_declared_bound_and_exported_at_abi_11(lib):
    hdr = open(os.path.join(ROOT, "include", "mapperhip.h")).read()
    assert re.search(r"\bint\s+mh_beam_step_path\s*\(\s*int num_beams,\s*int V,\s*int K\s*\)", hdr)
    assert re.search(r"#define\s+MH_ABI_VERSION\s+11\b", hdr)
    assert "mh_beam_step_path" in _lib.SYMBOLS and hasattr(lib, "mh_beam_step_path")
    assert _lib.ABI_VERSION == 11 and lib.mh_abi_version() == 11
    assert lib.mh_get_option(b"beam_step_path") == 0                      # automatic by default


LDS_SHAPES = [(2, 2080, 4), (7, 3837, 1024), (8, 3836, 16), (8, 512, 4096)]
STREAMING_SHAPES = [(8, 3837, 16), (8, 3839, 16), (7, 3837, 2048), (8, 3840, 16), (5, 8192, 10), (2, 3837, 5002), (8, 8192, 8192),
                    (2, 2080, 4097)]
REFUSED_SHAPES = [(9, 2080, 18), (1, 2080, 2), (8, 3837, 8193), (2, 2080, 1), (2, 3, 7)]    # beams, beams, K, K < beams, K > beams x V


def test_automatic_dispatch_keeps_the_lds_kernel_where_it_fits(lib):
    assert lib.mh_set_option(b"beam_step_path", 0) == 0
    for shape in LDS_SHAPES:
        assert lib.mh_beam_step_path(*shape) == 1, shape
    for shape in STREAMING_SHAPES:
        assert lib.mh_beam_step_path(*shape) == 2, shape
    for shape in REFUSED_SHAPES:
        assert lib.mh_beam_step_path(*shape) == 0, shape


def test_forced_paths(lib):
    assert lib.mh_set_option(b"beam_step_path", 1) == 0                   # the LDS kernel or nothing
    for shape in LDS_SHAPES:
        assert lib.mh_beam_step_path(*shape) == 1, shape
    for shape in STREAMING_SHAPES + REFUSED_SHAPES:
        assert lib.mh_beam_step_path(*shape) == 0, shape
    assert lib.mh_set_option(b"beam_step_path", 2) == 0                   # the streaming kernel wherever a step is accepted at all
    for shape in LDS_SHAPES + STREAMING_SHAPES:
        assert lib.mh_beam_step_path(*shape) == 2, shape
    for shape in REFUSED_SHAPES:
        assert lib.mh_beam_step_path(*shape) == 0, shape


def descriptor(num_beams, V, K):
    """Every pointer non-null (never dereferenced: the checks below fail on the numbers first)."""
    bs = _lib.MhBeamStep()
    for name, kind in _lib.MhBeamStep._fields_:
        if kind is _lib.VP:
            setattr(bs, name, 64)
    bs.G, bs.num_beams, bs.V, bs.P, bs.max_length, bs.K, bs.cur_len = 1, num_beams, V, 2, 24, K, 2
    bs.sp.temperature = 1.0
    return bs


def test_beam_step_names_the_limit_it_refuses_before_touching_anything(lib):
    assert lib.mh_beam_step(C.byref(descriptor(8, 3837, 8193)), None) == -1
    msg = lib.mh_last_error().decode()
    assert "K = 8193" in msg and "8192" in msg, msg
    assert lib.mh_beam_step(C.byref(descriptor(9, 3837, 18)), None) == -1
    msg = lib.mh_last_error().decode()
    assert "9 beams" in msg and "2 .. 8" in msg, msg
    assert lib.mh_set_option(b"beam_step_path", 1) == 0
    assert lib.mh_beam_step(C.byref(descriptor(8, 3837, 16)), None) == -1
    msg = lib.mh_last_error().decode()
    assert "8 x 3837" in msg and "120 KB" in msg and "beam_step_path" in msg, msg
    bs = descriptor(2, 2080, 4)
    bs.sp.do_sample = 1
    assert lib.mh_beam_step(C.byref(bs), None) == -1 and b"greedy beams only" in lib.mh_last_error()


def test_kernel_path_available_at_the_released_vocabulary(lib):
    from mapperatorinator_amd.beam import kernel_path_available
    greedy = types.SimpleNamespace(do_sample=0, lookback_types_first=0, lookback_mask_end=0, ts_start=0)
    assert kernel_path_available(greedy, 8, 3837, 2)                      # 122 784 B of scores: refused while LDS decided alone
    assert kernel_path_available(greedy, 5, 3837, 700) and kernel_path_available(greedy, 2, 3837, 2500)
    assert kernel_path_available(greedy, 2, 1849, 0)
    assert not kernel_path_available(greedy, 9, 3837, 2) and not kernel_path_available(greedy, 1, 3837, 2)
    assert not kernel_path_available(greedy, 8, 3837, 1024)               # K = 8200
    assert not kernel_path_available(types.SimpleNamespace(do_sample=1), 2, 1849, 0)
