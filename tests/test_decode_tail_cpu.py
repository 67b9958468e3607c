"""not gpu: the host side of the fused layer tail's bounded wait -- option, error code, and the mapping from the error word the
decode step leaves in its workspace to what mh_t5_generate returns (the timeout itself is never provoked on a device)."""
import os
import re

from mapperatorinator_amd import _lib


def test_decode_fused_tail_option_and_error_code_are_declared():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mapperhip.h")).read()
    assert re.search(r"MH_ERR_DECODE_TAIL_TIMEOUT\s*=\s*-4\b", hdr)
    assert re.search(r"\bint\s+mh_t5_decode_tail_status\s*\(\s*int err_word\s*\)", hdr)
    assert '"decode_fused_tail"' in hdr
    assert re.search(r"\blong\s+mh_t5_decode_tail_launches\s*\(\s*void\s*\)", hdr)
    assert _lib.load().mh_t5_decode_tail_launches() >= 0
    lib = _lib.load()
    assert lib.mh_get_option(b"decode_fused_tail") in (0, 1)
    old = lib.mh_get_option(b"decode_fused_tail")
    assert lib.mh_set_option(b"decode_fused_tail", 0) == 0 and lib.mh_get_option(b"decode_fused_tail") == 0
    assert lib.mh_set_option(b"decode_fused_tail", old) == 0


def test_tail_error_word_maps_to_timeout_status():
    lib = _lib.load()
    assert lib.mh_t5_decode_tail_status(0) == 0
    for word in (1, 7, -3):
        assert lib.mh_t5_decode_tail_status(word) == -4
        msg = lib.mh_last_error().decode()
        assert "decode_fused_tail" in msg and "2 ms" in msg and str(word) in msg, msg
