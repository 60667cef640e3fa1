"""The planned path's per-camera state over MANY views, with the state carried from view to view: the binding's LRU table of
plans and its graveyard (rasterizer.py _PLANS / _plan_entry / _retire / _PLAN_GRAVE), the recycled pinned plan_info blocks
(gsr_plan_info_free -> gsr_plan_info_new), the misfit back-off and the retry of an unplannable camera on real views, the binning
hint taken away and moved under a plan, two streams and both kinds of plan at once, and a miniature of the windowed refinement
loop.  The oracle is the project's own: a planned view equals the exact path (use_plan=False) on the same inputs -- image and radii
bit for bit, gradients to the order of the backward's float atomics (test_gpu_planned.py) -- what these tests add is stimulus, and
each asserts that it reached the path it is about.  Scenes: plan_scenes.py, proven on the CPU by test_plan_lifecycle_scenes.py
(every list below 1 024 entries but the unplannable one: above that the exact path may blend in parts, include/gsr.h)."""
import ctypes

import pytest
import torch

import plan_scenes as S
from test_gpu_planned import _check_same, _inputs, _render, _t

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _cam_t(cam):
    return dict(view=_t(cam.viewmatrix, DEV), proj=_t(cam.projmatrix, DEV), campos=_t(cam.campos, DEV))


def _verdict(delta):
    """What a view's PLAN_STATS delta says: binned by its plan / rendered the exact way because it outgrew it / the exact way
    with no plan to try / not handed a plan at all."""
    return "planned" if delta["planned"] else "misfit" if delta["misfit"] else "exact" if delta["exact"] else "left alone"


def _same(r, ref, what, worst):
    """_check_same, and worst[0] = the largest gradient gap seen (relative to the gradient's largest element)."""
    if r[2] is not None and ref[2] is not None:
        for ga, gb in zip(r[2], ref[2]):
            if ga is not None and ga.numel():
                worst[0] = max(worst[0], float((ga - gb).abs().max()) / max(float(gb.abs().max()), 1e-30))
    _check_same(r, ref, what)


def _blocks(rz):
    """{key: address of the pinned plan_info block} of the table right now (a function of its own: no _Plan outlives the call --
    a reference kept here would keep a retired plan's block from going back to the free list)."""
    return {k: ctypes.addressof(p.pi) for k, p in rz._PLANS.items()}


def _key(rz, cam, cam_t, need_backward=True, stream=0):
    """The table's key of a camera's plan, as _choose_plan makes it (the view matrix has been seen: a dictionary look-up)."""
    from gaustar_amd import _lib
    return (DEV.index, stream, cam.W, cam.H, need_backward, float(cam.tanfovx), float(cam.tanfovy),
            rz._camera_key(_lib.load(), cam_t["view"], DEV))


def _only_plan(rz):
    assert len(rz._PLANS) == 1, list(rz._PLANS)
    return next(iter(rz._PLANS.values()))


def _issue(rz, ps, cam_t, bg_t, cam, dpix, need_backward=True):
    """One view through the binding-level functions WITHOUT a host synchronisation: -> ((image, radii, grads or None), verdict)."""
    e = torch.Tensor([])
    before = dict(rz.PLAN_STATS)
    box = []
    R, color, radii, geom, binning, img, _maxc, nseg = rz.rasterize_gaussians_native(
        bg_t, ps["means3D"], ps["colors"], ps["opacities"], ps["scales"], ps["rotations"], 1.0, e, cam_t["view"], cam_t["proj"],
        cam.tanfovx, cam.tanfovy, cam.H, cam.W, e, 0, cam_t["campos"], False, False, need_backward=need_backward, scratch_box=box)
    delta = {k: rz.PLAN_STATS[k] - before[k] for k in before}
    grads = None
    if need_backward:
        grads = rz.rasterize_gaussians_backward_native(
            bg_t, ps["means3D"], radii, ps["colors"], ps["scales"], ps["rotations"], 1.0, e, cam_t["view"], cam_t["proj"], cam.tanfovx,
            cam.tanfovy, dpix, e, 0, cam_t["campos"], geom, R, binning, img, False, num_segments=nseg,
            zeroed_scratch=box[0] if box else None)
    return (color, radii, grads), _verdict(delta)


def _drained(rz):
    """Every plan gone and every block handed back: the end of each test."""
    torch.cuda.synchronize()
    rz.drop_plans()
    assert not rz._PLANS and not rz._PLAN_GRAVE, (len(rz._PLANS), len(rz._PLAN_GRAVE))


def _ring_inputs(n):
    """The static cloud through a ring of n cameras: -> (Gaussians on the device, cameras, their tensors, background, dL/dpixel,
    the exact path's result per camera).  The exact renders also leave the device a binning hint: without one a camera's first
    view leaves stage 2, and with it the plan, to the caller."""
    gs, cams = S.cloud(), S.ring(n)
    ps, _, bg_t, dpix = _inputs(DEV, gs, cams[0], S.BG)
    cam_ts = [_cam_t(c) for c in cams]
    exact = [_render(DEV, ps, cam_ts[c], bg_t, cams[c], dpix, use_plan=False) for c in range(n)]
    return ps, cams, cam_ts, bg_t, dpix, exact


# ------------------------------------------------------------------------------------------------ case 1
def test_eviction_with_the_device_idle_recycles_plans_and_blocks(monkeypatch):
    """Six cameras over a table of three, the device idle after every view.  (a) Bursts of three views per camera, four rounds:
    view 1 of a burst is exact -- the camera's plan has left the table since its last burst -- views 2 and 3 are planned.  (b)
    Round-robin, five rounds: LRU thrash, every view finds its camera's plan gone; none is planned, none misfits.

    Blocks.  _plan_entry drains the graveyard BEFORE it calls gsr_plan_info_new, and every retire event has passed by then (the
    helper synchronises after each view), so the drain drops the last reference to every retired plan and _Plan.__del__ has pushed
    its block back.  At that moment only the table's entries hold blocks: at most _PLAN_SLOTS.  The new entry makes it _PLAN_SLOTS
    + 1, the eviction loop moves one of them to the graveyard, where it keeps its block until the next drain.  The free list is a
    stack (g_pi_free: pop_back / push_back), and a stack hands out a block it has never handed out only when every block it ever
    handed out is in use -- so the number of distinct addresses equals the largest number of blocks held at once: _PLAN_SLOTS + 1,
    one more if the interpreter lets go of a drained plan a call late.  The bound asserted is that _PLAN_SLOTS + 2; a slab that
    leaked blocks would show one new address per evicted plan (dozens here)."""
    from gaustar_amd import rasterizer as rz
    rz.drop_plans()
    monkeypatch.setattr(rz, "_PLAN_SLOTS", 3)
    ps, cams, cam_ts, bg_t, dpix, exact = _ring_inputs(6)
    assert not rz._PLANS
    stats0 = dict(rz.PLAN_STATS)
    worst, keys_of_block, ever, entries, evictions = [0.0], {}, set(), [0], [0]

    def view(c, what):
        before = _blocks(rz)
        r = _render(DEV, ps, cam_ts[c], bg_t, cams[c], dpix)
        _same(r, exact[c], what, worst)
        now = _blocks(rz)
        assert len(now) <= 3, len(now)
        evictions[0] += len(set(before) - set(now))
        entries[0] += len(set(now) - set(before))
        mine = _key(rz, cams[c], cam_ts[c])
        assert mine in now
        for k, a in now.items():
            keys_of_block.setdefault(a, set()).add(k)
        had_plan, came_back = mine in before, mine in ever and mine not in before
        ever.update(now)
        return _verdict(r[3]), had_plan, came_back

    for rnd in range(4):
        for c in range(6):
            got = [view(c, f"burst {rnd}, camera {c}, view {i}") for i in range(3)]
            assert [g[0] for g in got] == ["exact", "planned", "planned"], (rnd, c, got)
            assert not got[0][1] and got[0][2] == (rnd > 0), (rnd, c, got)      # view 1: its plan was evicted since the last burst
    for rnd in range(5):
        for c in range(6):
            verdict, had_plan, came_back = view(c, f"round-robin {rnd}, camera {c}")
            assert verdict == "exact" and not had_plan and came_back, (rnd, c, verdict, had_plan, came_back)
    delta = {k: rz.PLAN_STATS[k] - stats0[k] for k in stats0}
    assert delta == {"planned": 4 * 6 * 2, "exact": 4 * 6 + 5 * 6, "misfit": 0}, delta
    assert entries[0] == 4 * 6 + 5 * 6 and evictions[0] == entries[0] - 3, (entries, evictions)     # a plan was evicted (51 were)
    assert len(keys_of_block) <= rz._PLAN_SLOTS + 2, sorted(keys_of_block)
    assert max(len(ks) for ks in keys_of_block.values()) >= 2                                         # a block address was reused
    print(f"[lifecycle] idle eviction: {entries[0]} plans made, {evictions[0]} evicted, {len(keys_of_block)} distinct plan_info blocks, "
          f"worst gradient gap {worst[0]:.2e}")
    _drained(rz)


# ------------------------------------------------------------------------------------------------ case 2
def test_eviction_with_builders_in_flight(monkeypatch):
    """The same six cameras over a table of three, two views per camera and five rounds, issued WITHOUT a host synchronisation
    between views: a camera's second view is planned and re-plans, and its plan leaves the table three cameras later while that
    builder may still be on its way to the plan's pinned block and plan buffer -- what the graveyard's events are for.  A block or a
    plan buffer recycled too early shows as a wrong image, as a misfit on a static scene, or as an error return."""
    from gaustar_amd import rasterizer as rz
    rz.drop_plans()
    monkeypatch.setattr(rz, "_PLAN_SLOTS", 3)
    ps, cams, cam_ts, bg_t, dpix, exact = _ring_inputs(6)
    torch.cuda.synchronize()
    outs, evictions, ever = [], 0, set()
    for rnd in range(5):
        for c in range(6):
            for i in range(2):
                before = set(rz._PLANS)
                out, verdict = _issue(rz, ps, cam_ts[c], bg_t, cams[c], dpix)
                evictions += len(before - set(rz._PLANS))
                assert len(rz._PLANS) <= 3
                ever.update(rz._PLANS)
                outs.append((rnd, c, i, out, verdict))
    torch.cuda.synchronize()
    worst = [0.0]
    for rnd, c, i, out, verdict in outs:
        assert verdict == ("planned" if i else "exact"), (rnd, c, i, verdict)       # no misfit; every second view by its plan
        _same(out, exact[c], f"in flight: round {rnd}, camera {c}, view {i}", worst)
    assert evictions == 5 * 6 - 3 and len(ever) == 6, (evictions, len(ever))          # plans were evicted with their builders under way
    print(f"[lifecycle] eviction in flight: {evictions} evicted, graveyard {len(rz._PLAN_GRAVE)} at the end, worst gradient gap {worst[0]:.2e}")
    del outs
    _drained(rz)


# ------------------------------------------------------------------------------------------------ case 3
def _policy(m, verdict):
    """The binding's back-off, restated from the verdicts alone: a paused camera is left alone and the pause counts down; a
    planned view ends a run of misfits; a misfit raises the slack level (at most 3) and, from the second in a row on, pauses the
    camera for min(64, 2^(misfits - 1)) views."""
    if m["skip"] > 0:
        assert verdict == "left alone", (verdict, m)
        m["skip"] -= 1
        return
    assert verdict != "left alone", m
    if verdict == "planned":
        m["misfits"] = 0
    elif verdict == "misfit":
        m["misfits"] += 1
        m["level"] = min(m["level"] + 1, 3)
        if m["misfits"] >= 2:
            m["skip"] = min(64, 1 << (m["misfits"] - 1))


def test_misfit_back_off_on_the_device():
    """One camera; a cluster of 600 Gaussians visits the four image corners in turn, 40 visits.  A corner's tiles, and their
    neighbours, were empty in the view before (test_plan_lifecycle_scenes.py): capacity 0 at any slack level, so every view that
    tries its plan outgrows it -- misfits in a row, pauses of 2, 4, 8, .. views.  After every view the binding's misfits / skip /
    level equal _policy's.  Then the cluster is held still: once the pause is over the camera is planned again."""
    from gaustar_amd import rasterizer as rz
    rz.drop_plans()
    cam = S.camera()
    cam_t = _cam_t(cam)
    ins = [_inputs(DEV, S.corner_cluster(v), cam, S.BG) for v in range(len(S.CORNERS))]
    bg_t, dpix = ins[0][2], ins[0][3]
    exact = [_render(DEV, ins[v][0], cam_t, bg_t, cam, dpix, use_plan=False) for v in range(len(ins))]    # (and the binning hint)
    model = dict(misfits=0, skip=0, level=int(rz._PLAN_LEVEL_ENV) if rz._PLAN_LEVEL_ENV is not None else 1)
    worst, verdicts, row, longest_skip = [0.0], [], 0, 0

    def visit(v, what):
        r = _render(DEV, ins[v][0], cam_t, bg_t, cam, dpix)
        _same(r, exact[v], what, worst)
        verdict = _verdict(r[3])
        _policy(model, verdict)
        plan = _only_plan(rz)
        assert (plan.misfits, plan.skip, plan.pi.level) == (model["misfits"], model["skip"], model["level"]), (what, verdict, model)
        verdicts.append(verdict)
        return verdict

    for n in range(40):
        verdict = visit(n % len(ins), f"corner visit {n}")
        assert verdict != "planned", (n, verdicts)          # (the cluster is never where the plan has room)
        row = max(row, model["misfits"])
        longest_skip = max(longest_skip, model["skip"])
    assert verdicts[0] == "exact" and row >= 3 and longest_skip >= 4, (row, longest_skip, verdicts)
    moving = list(verdicts)
    # held still: whatever is left of the pause, at most one more misfit (the plan under way is of another corner) and its pause
    # of at most 64 views, one exact view that leaves a plan of THIS corner, then planned
    still = 39 % len(ins)
    for k in range(model["skip"] + 1 + 64 + 1 + 2):
        if visit(still, f"held still, view {k}") == "planned" and verdicts[-2] == "planned":
            break
    held = verdicts[len(moving):]
    assert held[-2:] == ["planned", "planned"] and held.count("misfit") <= 1, held
    assert model["misfits"] == 0 and model["skip"] == 0
    print(f"[lifecycle] back-off: moving {''.join(v[0] for v in moving)}, held still {''.join(v[0] for v in held)} "
          f"(p planned, e exact, m misfit, l left alone); misfits in a row {row}, longest pause {longest_skip}, "
          f"worst gradient gap {worst[0]:.2e}")
    _drained(rz)


# ------------------------------------------------------------------------------------------------ case 4
def test_unplannable_camera_is_asked_again_and_planned_once_it_fits():
    """64 x 64 pixels, 2 200 Gaussians on the image centre: the centre tiles' lists are above PLAN_MAX_LIST - 16 (proven on the
    CPU), so the first view marks the camera unplannable (state -1) and every view is exact -- the planned call and the exact
    reference take the same exact path, lists above 2 048 entries included.  After _PLAN_RETRY such views the binding asks again
    (state 0).  Cut to its first 800 Gaussians the scene fits: the next view leaves a plan, the ones after it are planned."""
    from gaustar_amd import rasterizer as rz
    rz.drop_plans()
    gs, cam = S.unplannable()
    cam_t = _cam_t(cam)
    ps, _, bg_t, dpix = _inputs(DEV, gs, cam, S.BG)
    exact = _render(DEV, ps, cam_t, bg_t, cam, dpix, use_plan=False)
    assert exact[4][0] == 4 * S.UNPLANNABLE_P, exact[4]
    worst = [0.0]
    assert rz._PLAN_RETRY == 32
    for n in range(1, rz._PLAN_RETRY + 1):
        r = _render(DEV, ps, cam_t, bg_t, cam, dpix)
        _same(r, exact, f"unplannable view {n}", worst)
        plan = _only_plan(rz)
        assert _verdict(r[3]) == "exact" and plan.pi.pending == 0, (n, r[3])
        if n < rz._PLAN_RETRY:
            assert plan.pi.state == -1 and plan.idle == n, (n, plan.pi.state, plan.idle)       # state was -1 ...
        else:
            assert plan.pi.state == 0 and plan.idle == 0, (plan.pi.state, plan.idle)           # ... and returned to 0
    small, _, _, _ = _inputs(DEV, S.cut(gs, S.CUT_P), cam, S.BG)
    exact_small = _render(DEV, small, cam_t, bg_t, cam, dpix, use_plan=False)
    got = []
    for n in range(4):
        r = _render(DEV, small, cam_t, bg_t, cam, dpix)
        _same(r, exact_small, f"cut scene, view {n}", worst)
        got.append(_verdict(r[3]))
        plan = _only_plan(rz)
        assert plan.pi.state == (0 if n == 0 else 1) and plan.idle == 0, (n, plan.pi.state)
    assert got == ["exact", "planned", "planned", "planned"], got
    print(f"[lifecycle] unplannable: worst gradient gap {worst[0]:.2e}")
    _drained(rz)


# ------------------------------------------------------------------------------------------------ case 5
def test_binning_hint_taken_away_and_moved_under_a_plan(monkeypatch):
    """Two cameras in steady planned views.  The device's binning hint set to 0 under a VALID plan: has_usable_plan says no (no
    binning buffer), exact_view ends in hand_back_counters, the library returns blended == 0 and the caller runs stage 2 over an
    exactly sized buffer -- seen here as the binding's one call of gsr_forward_stage2_mt -- no plan job rides, the plan stays valid
    and the next view is planned again.  Then one 1080p view of config C makes the hint jump, and the small cameras go on planned
    and correct while it comes down: after every view the hint is _next_hint of the hint before and the bytes the view reports."""
    from gaustar_amd import _lib, rasterizer as rz, scene
    lib = _lib.load()
    rz.drop_plans()
    ps, cams, cam_ts, bg_t, dpix, exact = _ring_inputs(2)
    worst = [0.0]
    stage2 = []
    real_stage2 = lib.gsr_forward_stage2_mt
    monkeypatch.setattr(lib, "gsr_forward_stage2_mt", lambda *a: stage2.append(1) or real_stage2(*a))

    def key_of(c):
        return _key(rz, cams[c], cam_ts[c])

    def state_of(c):
        pi = rz._PLANS[key_of(c)].pi
        return pi.state, pi.pending

    def hint():
        with rz._HINT_LOCK:
            return rz._BINNING_HINT.get(DEV.index, 0)

    def view(c, what):
        """-> (verdict, the bytes the view reports: _need_bytes of its sizes and its camera's plan)"""
        r = _render(DEV, ps, cam_ts[c], bg_t, cams[c], dpix)
        _same(r, exact[c], what, worst)
        return _verdict(r[3]), rz._need_bytes(lib.gsr_binning_bytes_mt, 3, r[4][0], r[4][1], rz._PLANS[key_of(c)].pi)

    for rnd in range(3):
        got = [view(c, f"warm-up {rnd}, camera {c}")[0] for c in range(2)]
    assert got == ["planned", "planned"] and not stage2, (got, stage2)
    for c in range(2):
        with rz._HINT_LOCK:
            rz._BINNING_HINT[DEV.index] = 0
        assert state_of(c)[0] == 1
        verdict, need = view(c, f"no hint, camera {c}")
        # blended == 0 under a valid plan: stage 2 was the caller's, nothing was planned or re-planned, the plan is still valid
        assert verdict == "exact" and len(stage2) == c + 1 and state_of(c) == (1, 0), (c, verdict, stage2, state_of(c))
        assert hint() == rz._next_hint(0, need) > 0, (hint(), need)
    for rnd in range(3):
        got = [view(c, f"hint back {rnd}, camera {c}")[0] for c in range(2)]
    assert got == ["planned", "planned"] and len(stage2) == 2, (got, stage2)

    gs_c, cams_c, bg_c = scene.config_C()
    ps_c, cam_c_t, bg_c_t, dpix_c = _inputs(DEV, gs_c, cams_c[0], bg_c)
    before = hint()
    big = _render(DEV, ps_c, cam_c_t, bg_c_t, cams_c[0], dpix_c)
    need_c = int(lib.gsr_binning_bytes_mt(big[4][0], big[4][1], 3))
    assert hint() == rz._next_hint(before, need_c) > before, (before, need_c, hint())          # the hint jumped
    _check_same(big, _render(DEV, ps_c, cam_c_t, bg_c_t, cams_c[0], dpix_c, use_plan=False), "the 1080p view")
    del ps_c, big
    hints = [hint()]
    for n in range(20):
        verdict, need = view(n % 2, f"under the moving hint, view {n}")
        assert verdict == "planned", (n, verdict)
        assert hint() == rz._next_hint(hints[-1], need), (n, hints, need, hint())
        hints.append(hint())
    assert hints[-1] < hints[0] and len(set(hints)) >= 3, hints                                  # it came down, in steps
    assert all(a >= b for a, b in zip(hints, hints[1:])), hints
    print(f"[lifecycle] hint: {[h >> 20 for h in hints]} MB, worst gradient gap {worst[0]:.2e}")
    _drained(rz)


# ------------------------------------------------------------------------------------------------ case 6
def test_two_streams_and_two_kinds_of_plan_interleaved():
    """Four cameras, ten rounds; every camera is rendered differentiably on stream A and forward-only on stream B, the two
    streams' calls interleaved from one host thread with no synchronisation until the end.  Stream and kind are part of a plan's
    key: eight plans, each exact in round 0 and planned from then on; the library's cursor and counter blocks are per stream."""
    from gaustar_amd import rasterizer as rz
    rz.drop_plans()
    ps, cams, cam_ts, bg_t, dpix, exact = _ring_inputs(4)
    torch.cuda.synchronize()
    a, b = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    outs = []
    for rnd in range(10):
        for c in range(4):
            with torch.cuda.stream(a):
                outs.append((rnd, c, "differentiable, stream A") + _issue(rz, ps, cam_ts[c], bg_t, cams[c], dpix))
            with torch.cuda.stream(b):
                outs.append((rnd, c, "forward-only, stream B") + _issue(rz, ps, cam_ts[c], bg_t, cams[c], None, need_backward=False))
    torch.cuda.synchronize()
    keys = list(rz._PLANS)
    assert len(keys) == 8 and {(k[1], k[4]) for k in keys} == {(a.cuda_stream, True), (b.cuda_stream, False)}, keys
    assert a.cuda_stream != b.cuda_stream and 0 not in (a.cuda_stream, b.cuda_stream)
    worst = [0.0]
    planned = {"differentiable, stream A": 0, "forward-only, stream B": 0}
    for rnd, c, kind, out, verdict in outs:
        assert verdict == ("planned" if rnd else "exact"), (rnd, c, kind, verdict)          # no misfit; planned from round 2 on
        planned[kind] += verdict == "planned"
        _same(out, exact[c], f"round {rnd}, camera {c}, {kind}", worst)
    assert planned == {"differentiable, stream A": 36, "forward-only, stream B": 36}, planned   # both streams, both kinds of plan
    print(f"[lifecycle] two streams: planned {planned}, worst gradient gap {worst[0]:.2e}")
    del outs
    _drained(rz)


# ------------------------------------------------------------------------------------------------ case 7
def test_soak_windowed_loop_in_miniature(monkeypatch):
    """Config E in miniature (plan_scenes.Soak): eight cameras over a table of five, 40 frames of 12 iterations, the Gaussians
    drifting within a frame and jumping at its boundary, the scales breathing -- 480 iterations, each rendered planned with backward
    and exact with backward on the same inputs and compared.  Planned fraction and misfit count are printed, not asserted: nobody
    has measured them for this scene."""
    from gaustar_amd import rasterizer as rz
    rz.drop_plans()
    monkeypatch.setattr(rz, "_PLAN_SLOTS", 5)
    handed = []
    choose = rz._choose_plan

    def spy(*a, **kw):       # (whether the binding handed this view a plan at all: a paused camera's view gets None)
        plan = choose(*a, **kw)
        handed.append(plan is not None)
        return plan

    monkeypatch.setattr(rz, "_choose_plan", spy)
    soak = S.Soak()
    ps, _, bg_t, dpix = _inputs(DEV, soak.gs, soak.cams[0], S.BG)
    cam_ts = [_cam_t(c) for c in soak.cams]
    stats0 = dict(rz.PLAN_STATS)
    worst, tally, with_plan, evictions = [0.0], {"planned": 0, "exact": 0, "misfit": 0, "left alone": 0}, 0, 0
    for frame in range(S.SOAK_FRAMES):
        for it in range(S.SOAK_ITERS):
            c = soak.camera_of(frame, it)
            means, scales = soak.gaussians(frame, it)
            moved = dict(ps, means3D=_t(means, DEV), scales=_t(scales, DEV))
            exact = _render(DEV, moved, cam_ts[c], bg_t, soak.cams[c], dpix, use_plan=False)
            before, calls = set(rz._PLANS), len(handed)
            r = _render(DEV, moved, cam_ts[c], bg_t, soak.cams[c], dpix)
            _same(r, exact, f"soak frame {frame}, iteration {it}, camera {c}", worst)
            assert len(rz._PLANS) <= 5 and len(handed) == calls + 1
            evictions += len(before - set(rz._PLANS))
            with_plan += handed[-1]
            verdict = _verdict(r[3])
            assert (verdict != "left alone") == handed[-1], (frame, it, verdict)
            tally[verdict] += 1
    delta = {k: rz.PLAN_STATS[k] - stats0[k] for k in stats0}
    print(f"[lifecycle] soak: {tally} of {S.SOAK_FRAMES * S.SOAK_ITERS} views, {evictions} plans evicted, "
          f"worst gradient gap {worst[0]:.2e}")
    assert delta["planned"] + delta["exact"] == with_plan and delta["misfit"] <= delta["exact"], (delta, with_plan)
    assert delta == {"planned": tally["planned"], "exact": tally["exact"] + tally["misfit"], "misfit": tally["misfit"]}, (delta, tally)
    assert tally["planned"] >= 1 and evictions >= 1, (tally, evictions)
    _drained(rz)
