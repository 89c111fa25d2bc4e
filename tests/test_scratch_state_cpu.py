"""Static checks of gnx_debug_fill_scratch (gonomics_amd/csrc/gnx_align.hip): the hook that dirties the workspace between two calls
(tests/test_scratch_state_gpu.py).

CPU-only.  The hook names every device and pinned buffer of `struct Ctx` in one of two lists -- SCRATCH, filled over its whole
capacity, and STATE, filled behind what its owner wrote.  A buffer that a later change adds to Ctx and to neither list would stay
clean for ever, and whatever reads it unwritten would stay unseen; a buffer named in both would lose state.  So `struct Ctx` is parsed
from the source, arrays included, and every DevBuf / PinBuf member must be named in exactly one list.  The hook is a test hook: without
GNX_DEBUG_ENTRY it is refused before it looks for a device."""
import os
import re

import pytest

from gonomics_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gonomics_amd", "csrc", "gnx_align.hip")

# what the issue of the hook names as state: the resident reference, the reference k-mer index, the graph seed index, the open pile
STATE = {"ref", "ref_flag", "ref_rank", "ref_exc", "ri_keys", "ri_pos", "ri_dir", "sd_keys", "sd_locs", "sd_nodes", "sd_node_off", "sd_word_off",
         "sd_words", "pl_tab", "pl_log", "pl_cur", "pl_qsum"}


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def ctx_members(src):
    """{member: (type, array length or None)} of the DevBuf / PinBuf members of struct Ctx"""
    m = re.search(r"\nstruct Ctx \{\n(.*?)\n\};", src, flags=re.S)
    assert m, "struct Ctx not found"
    out = {}
    for typ, decl in re.findall(r"\b(DevBuf|PinBuf)\s+([^;]*);", strip_comments(m.group(1))):
        for item in decl.split(","):
            mm = re.fullmatch(r"\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*", item)
            assert mm, "unparsed declarator %r" % item
            assert mm.group(1) not in out, "declared twice: " + mm.group(1)
            out[mm.group(1)] = (typ, int(mm.group(2)) if mm.group(2) else None)
    return out


def hook_lists(src):
    """(names in the scratch list, names in the state list, array members the hook walks with a range-for), each with multiplicity"""
    m = re.search(r"\nint gnx_debug_fill_scratch\(.*?\n\}\n", src, flags=re.S)
    assert m, "gnx_debug_fill_scratch not found"
    body = m.group(0)

    def region(tag):
        r = re.search(r"\[%s-list-begin\](.*?)// \[%s-list-end\]" % (tag, tag), body, flags=re.S)
        assert r, tag + " list markers not found"
        return strip_comments(r.group(1))
    scratch, state = region("scratch"), region("state")
    names = lambda text: re.findall(r"\bc\.(\w+)\b(?!\s*\()", text)
    loops = re.findall(r"for\s*\(\s*(?:DevBuf|PinBuf)\s*&\s*\w+\s*:\s*c\.(\w+)\s*\)", scratch + state)
    return names(scratch), names(state), set(loops)


NOT_BUFFERS = {"ref_len", "ref_nexc", "ri_n", "ri_dir_bits", "sd_n", "sd_total", "sd_nodes_n", "sd_words_n", "pl_len", "pl_qual", "pl_track", "pl_log_cap",
               "pl_events"}  # the scalars the state list takes its used sizes from


def test_ctx_is_parsed():
    mem = ctx_members(open(SRC).read())
    assert len(mem) >= 100 and mem["trace"] == ("DevBuf", None) and mem["sm"] == ("DevBuf", 14) and mem["st_a"] == ("PinBuf", 2) and mem["h_plans"] == ("PinBuf", None)
    assert sum(n or 1 for t, n in mem.values() if t == "DevBuf") >= 150
    assert STATE <= set(mem)


def test_every_buffer_is_classified_exactly_once():
    src = open(SRC).read()
    mem = ctx_members(src)
    scratch, state, loops = hook_lists(src)
    scratch = [n for n in scratch if n not in NOT_BUFFERS]
    state_names = [n for n in state if n not in NOT_BUFFERS]
    for n in scratch + state_names:
        assert n in mem, "the hook names c.%s, which is no DevBuf / PinBuf of Ctx" % n
    assert len(scratch) == len(set(scratch)), "named twice in the scratch list: %s" % sorted(n for n in set(scratch) if scratch.count(n) > 1)
    assert set(state_names) == STATE, (sorted(set(state_names) - STATE), sorted(STATE - set(state_names)))
    both = set(scratch) & set(state_names)
    assert not both, "named as scratch and as state: %s" % sorted(both)
    missing = sorted(set(mem) - set(scratch) - set(state_names))
    assert not missing, "buffers of Ctx the hook does not classify (scratch: filled whole; state: filled behind its used part): %s" % missing
    # an array is walked whole: a range-for over the member, never single elements
    arrays = {n for n, (_, k) in mem.items() if k is not None}
    assert arrays <= loops, "arrays not walked with a range-for: %s" % sorted(arrays - loops)
    assert loops <= arrays


def test_an_unclassified_buffer_is_noticed():
    """the check above must fail for a member that a later change adds: a copy of the source with one more DevBuf in Ctx"""
    src = open(SRC).read()
    grown = src.replace("    PinBuf h_plans;", "    DevBuf brand_new, brand_arr[3];\n    PinBuf h_plans;", 1)
    assert grown != src
    mem = ctx_members(grown)
    scratch, state, _ = hook_lists(grown)
    assert sorted(set(mem) - set(scratch) - set(state)) == ["brand_arr", "brand_new"]


def test_the_hook_drops_the_plan_cache_and_checks_its_fills():
    src = open(SRC).read()
    body = re.search(r"\nint gnx_debug_fill_scratch\(.*?\n\}\n", src, flags=re.S).group(0)
    assert "c.fpc_ptr = nullptr;" in body
    assert "hipMemsetD32Async" in body and "hipStreamSynchronize" in body and "did not land" in body
    assert body.index('getenv("GNX_DEBUG_ENTRY")') < body.index("ctx_at(")  # refused before any context is touched


def test_entry_is_a_test_hook(monkeypatch):
    monkeypatch.delenv("GNX_DEBUG_ENTRY", raising=False)
    with pytest.raises(_lib.GnxError) as e:
        _lib.debug_fill_scratch(0x80808080)
    assert e.value.code == _lib.GNX_EINVAL and "GNX_DEBUG_ENTRY" in str(e.value)
