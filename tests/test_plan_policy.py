"""The planned forward's host side without a GPU: the plan_info block has ONE layout (include/gsr.h's gsr_plan_info, mirrored by
_lib.PlanInfo), and the binding's policies -- the binning hint, what a plan does after a view -- are functions of plain values."""
import ctypes
import os
import re

from conftest import ROOT

MB = 1 << 20


def _header_struct():
    """-> ([(field, number of ints)], GSR_PLAN_INFO_INTS) as include/gsr.h declares them."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsr.h")).read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s+gsr_plan_info\s*\{(.*?)\}\s*gsr_plan_info\s*;", src, flags=re.S).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(r"int\s+(\w+)\s*(?:\[\s*(\d+)\s*\])?", decl)
        assert m, f"gsr_plan_info holds ints only, got {decl!r}"
        fields.append((m.group(1), int(m.group(2) or 1)))
    return fields, int(re.search(r"#define\s+GSR_PLAN_INFO_INTS\s+(\d+)", src).group(1))


def test_plan_info_struct_is_the_header_s():
    from gaustar_amd import _lib
    fields, ints = _header_struct()
    mirror = [(name, ctypes.sizeof(t) // ctypes.sizeof(ctypes.c_int)) for name, t in _lib.PlanInfo._fields_]
    assert fields == mirror
    assert [name for name, _ in fields[:7]] == ["state", "R_cap", "U_cap", "max_cap", "level", "half", "pending_half"]
    assert ctypes.sizeof(_lib.PlanInfo) == 4 * ints == 4 * _lib.PLAN_INFO_INTS == 4 * sum(n for _, n in fields)


def test_plan_info_words_show_up_in_their_fields():
    """Word k written through the int pointer the library takes reads back from the field the layout puts there."""
    from gaustar_amd import _lib
    words = (ctypes.c_int * _lib.PLAN_INFO_INTS)()
    raw = ctypes.cast(words, ctypes.POINTER(ctypes.c_int))
    pi = ctypes.cast(raw, ctypes.POINTER(_lib.PlanInfo)).contents
    named = {0: "state", 1: "R_cap", 2: "U_cap", 3: "max_cap", 4: "level", 5: "half", 6: "pending_half", 16: "arrived", 17: "pending"}
    named.update({8 + i: ("header", i) for i in range(8)})
    named.update({18 + i: ("diag", i) for i in range(4)})
    for k, where in named.items():
        raw[k] = 1000 + k
        got = getattr(pi, where) if isinstance(where, str) else getattr(pi, where[0])[where[1]]
        assert got == 1000 + k, (k, where)
        offset = getattr(_lib.PlanInfo, where if isinstance(where, str) else where[0]).offset
        assert offset == 4 * (k if isinstance(where, str) else k - where[1]), (k, where)
    assert (_lib.PH_VALID, _lib.PH_T, _lib.PH_R_CAP, _lib.PH_U_CAP, _lib.PH_MAX_CAP) == (0, 1, 2, 3, 4)


def test_binning_hint_policy():
    from gaustar_amd.rasterizer import _next_hint
    assert _next_hint(0, 1) == 32 * MB
    assert _next_hint(256 * MB, 64 * MB) == 256 * MB            # 4 * 64 is not below 256
    assert _next_hint(256 * MB, 60 * MB) == 128 * MB            # the larger of ceil32(75) and ceil32(128)
    assert _next_hint(64 * MB, 100 * MB) == 128 * MB            # need above current: ceil32(1.25 * need)
    assert _next_hint(64 * MB, 64 * MB + 1) == 96 * MB
    assert _next_hint(64 * MB, 64 * MB) == 64 * MB


def test_need_bytes_counts_the_plan_in_use_and_the_one_that_has_landed():
    from gaustar_amd import _lib
    from gaustar_amd.rasterizer import _need_bytes
    size = lambda R, U, C: 100 * R + U + C
    pi = _lib.PlanInfo()
    assert _need_bytes(size, 3, 10, 2) == 1005 == _need_bytes(size, 3, 10, 2, pi)      # no valid plan: the view's own need
    pi.state, pi.R_cap, pi.U_cap = 1, 64, 1
    assert _need_bytes(size, 3, 10, 2, pi) == 6404
    pi.header[_lib.PH_VALID], pi.header[_lib.PH_R_CAP], pi.header[_lib.PH_U_CAP] = 1, 128, 2
    pi.arrived, pi.pending = 4, 5                                # (still on its way)
    assert _need_bytes(size, 3, 10, 2, pi) == 6404
    pi.arrived = 5
    assert _need_bytes(size, 3, 10, 2, pi) == 12805
    pi.pending = 0                                              # (adopted already: R_cap / U_cap say it)
    assert _need_bytes(size, 3, 10, 2, pi) == 6404


def _plan():
    from gaustar_amd import _lib
    from gaustar_amd.rasterizer import _Plan
    words = (ctypes.c_int * _lib.PLAN_INFO_INTS)()
    plan = _Plan(ctypes.cast(words, ctypes.POINTER(ctypes.c_int)), level=1)
    assert words[4] == 1 and plan.pi.level == 1
    return plan, words


def test_misfits_in_a_row_pause_planning():
    plan, _ = _plan()
    skips = []
    for _ in range(8):
        plan.skip = 0
        plan.after_view(-1)
        skips.append(plan.skip)
    assert [skips[n - 1] for n in (1, 2, 3, 7, 8)] == [0, 2, 4, 64, 64]
    plan.skip = 0
    plan.after_view(1)                 # a planned view resets the run
    plan.after_view(-1)
    assert plan.misfits == 1 and plan.skip == 0
    plan.after_view(0)                 # (an exact view without a misfit leaves it standing)
    plan.after_view(-1)
    assert plan.misfits == 2 and plan.skip == 2


def test_unplannable_camera_is_asked_again_after_32_views():
    from gaustar_amd.rasterizer import _PLAN_RETRY, PLAN_STATS
    assert _PLAN_RETRY == 32
    plan, words = _plan()
    before = dict(PLAN_STATS)
    words[0] = -1
    for n in range(1, 32):
        plan.after_view(0)
        assert words[0] == -1 and plan.idle == n
    plan.after_view(0)
    assert words[0] == 0 and plan.idle == 0
    assert {k: PLAN_STATS[k] - before[k] for k in before} == {"planned": 0, "exact": 32, "misfit": 0}
