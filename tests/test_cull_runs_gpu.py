"""The crafted runs of tests/cull_runs_cases.py through every search -- k_lsd (the per-call trait path and the classic batch), k_lsd_tile
(FrameBatch), k_lsd_service (a frame-granular pipeline at 1024 x 768, plain and without team help) and k_lsd_service_c (the same at
2560 x 1440) -- at the thresholds 15, 23, 24, 47 and 48: both sides of smh_cull_by_runs (csrc/smh_cull_rule.h), for the middle annulus
(23 | 24) and for the outer one (47 | 48).

  * lines, n_lines, rounds and n_mask_px are the oracle's, byte for byte;
  * under STAGE_EXACT_STATS ray_steps is the oracle's;
  * without exact statistics ray_steps is at most the oracle's and the SAME in every search (one rule, whichever kernel scans);
  * for the blob with an arc 40 px away ray_steps is strictly below the exact run's wherever the rule can drop a unit of the blob's
    candidate.  That is asserted on the CPU first (the header's table over the oracle's mask, cull_chain_cases.live_units): at the
    thresholds 15, 23 and 24 the blob's own pixels lie below the outer annulus and units are dropped; at 47 and 48 the outer annulus
    starts at step 3 | 2, holds the blob's own pixels, whose codes stand for every unit, and nothing of that candidate can be dropped.

Every claim a case makes about its mask (the runs, the blob the offsets count from) is asserted on the oracle's mask when the reference is
computed (cull_runs_cases.reference)."""
import numpy as np
import pytest

import cull_chain_cases as CC
import cull_runs_cases as RC

pytestmark = pytest.mark.gpu

SIZE_IDS = {RC.SIZES[0]: "768p", RC.SIZES[1]: "1440p"}
COMBOS = [(s_, t) for s_ in RC.SIZES for t in RC.MAX_GAPS]
COMBO_IDS = ["%s-gap%d" % (SIZE_IDS[s_], t) for s_, t in COMBOS]


@pytest.fixture(scope="module")
def frames():
    """size -> frames on the device; (size, max_gap) -> (names, [Ref]): the oracle's answers once per session."""
    import torch
    held = {}

    def get(size, max_gap):
        names = [c.name for c in RC.cases()]
        if size not in held:
            held[size] = torch.from_numpy(np.stack([RC.frame(c, *size) for c in RC.cases()])).cuda()
        refs = RC.reference(size, max_gap)
        return names, [refs[n] for n in names], held[size]

    yield get
    held.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def strict(tmp_path_factory):
    """max_gap -> does the rule drop a unit of the blob's candidate in arc_outer_only?  On the CPU: the condensed table (the byte codes
    the device holds) over the oracle's mask, the outer annulus alone -- the chain can only drop more."""
    import test_cull_runs_host as TH
    exe = TH.checker(tmp_path_factory.mktemp("cull_runs_gpu"))
    out = {}
    for t in RC.MAX_GAPS:
        in_o, _, units = RC.coded_table(exe, t)
        R = RC.reference(RC.SIZES[0], t)["arc_outer_only"]
        ys, xs = np.nonzero(R.mask == 255)
        out[t] = RC.seen_units(R.mask, int(xs[0]), int(ys[0]) + 1, in_o, units) != (1 << CC.UNITS) - 1   # (the blob's first pixel is (0, -1) from its start point's pixel)
    assert out == {15: True, 23: True, 24: True, 47: False, 48: False}, out
    return out


@pytest.fixture(scope="module")
def culled_steps():
    """(size, max_gap) -> {search: [ray_steps per case]} of the culled runs, filled by the tests below and compared by the last one."""
    return {}


def _check(got, refs, exact, strict_here, tag):
    assert len(got) == len(refs)
    for g, R in zip(got, refs):
        name = R.case.name
        assert g["n_lines"] == len(R.lines) and np.array_equal(g["lines"], R.lines), (name, g["lines"], R.lines) + tag
        assert g["rounds"] == R.rounds and g["n_mask_px"] == R.n_mask_px, (name, g["rounds"], R.rounds, g["n_mask_px"], R.n_mask_px) + tag
        if exact:
            assert g["ray_steps"] == R.steps, (name, g["ray_steps"], R.steps) + tag
        else:
            assert g["ray_steps"] <= R.steps, (name, g["ray_steps"], R.steps) + tag
            if name == "arc_outer_only" and strict_here:
                assert g["ray_steps"] < R.steps, (name, g["ray_steps"], R.steps) + tag


@pytest.mark.parametrize("size,max_gap", COMBOS, ids=COMBO_IDS)
def test_per_call_trait_path(vision, frames, strict, culled_steps, size, max_gap):
    import squad_mortar_helper_amd as smh
    names, refs, d = frames(size, max_gap)
    steps = []
    st = smh.VisionState(grayscale_map=True, max_gap=max_gap)
    try:
        for i, R in enumerate(refs):
            res = st.process(vision, d[i].cpu().numpy())
            assert np.array_equal(vision.lsd_image(), R.mask), names[i]
            assert res.markers.shape == R.lines.shape and np.array_equal(res.markers, R.lines), (names[i], res.markers, R.lines)
            r_fast, s_fast = vision.lsd_stats(max_gap, exact=False)
            r_exact, s_exact = vision.lsd_stats(max_gap, exact=True)
            assert r_fast == r_exact == R.rounds and s_exact == R.steps and s_fast <= s_exact, (names[i], r_fast, r_exact, R.rounds, s_fast, s_exact, R.steps)
            if names[i] == "arc_outer_only" and strict[max_gap]:
                assert s_fast < s_exact, (s_fast, s_exact)
            steps.append(s_fast)
    finally:
        st.close()
    culled_steps.setdefault((size, max_gap), {})["per_call"] = steps


@pytest.mark.parametrize("variant", ("default", "classic"))
@pytest.mark.parametrize("size,max_gap", COMBOS, ids=COMBO_IDS)
def test_frame_batch(vision, frames, strict, culled_steps, size, max_gap, variant):
    import torch
    import squad_mortar_helper_amd as smh
    lib = smh._lib.load()
    names, refs, d = frames(size, max_gap)
    fb = smh.FrameBatch(vision, size[0], size[1], len(refs))
    try:
        lib.smhv_debug_lsd_classic(int(variant == "classic"))
        for exact in (0, smh.STAGE_EXACT_STATS):
            fb.run(d.data_ptr(), len(refs), stages=smh.STAGE_MARKERS | exact, max_gap=max_gap, stream=torch.cuda.current_stream().cuda_stream)
            got = smh.results_to_dicts(fb.read_results(0, len(refs)))
            _check(got, refs, exact, strict[max_gap], (variant, bool(exact)))
            if not exact:
                culled_steps.setdefault((size, max_gap), {})["batch_" + variant] = [g["ray_steps"] for g in got]
    finally:
        lib.smhv_debug_lsd_classic(0)
        fb.close()


@pytest.mark.parametrize("variant", ("plain", "no_team_help"))
@pytest.mark.parametrize("size,max_gap", COMBOS, ids=COMBO_IDS)
def test_search_service(vision, frames, strict, culled_steps, size, max_gap, variant):
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib
    names, refs, d = frames(size, max_gap)
    pipe = smh.Pipeline(vision, size[0], size[1], len(refs), 3, search="frame", flags=_lib.PIPE_NO_TEAM_HELP if variant == "no_team_help" else 0)
    try:
        assert pipe.peek()["service_workgroups"] > 0
        for exact in (0, smh.STAGE_EXACT_STATS):
            slots = [pipe.submit(d.data_ptr(), len(refs), stages=smh.STAGE_MARKERS | exact, max_gap=max_gap) for _ in range(3)]
            pipe.wait()
            for s_ in sorted(set(slots)):
                got = smh.results_to_dicts(pipe.slots[s_].read_results(0, len(refs)))
                _check(got, refs, exact, strict[max_gap], (variant, bool(exact), s_))
                if not exact:
                    culled_steps.setdefault((size, max_gap), {})["service_%s_%d" % (variant, s_)] = [g["ray_steps"] for g in got]
    finally:
        pipe.close()


@pytest.mark.parametrize("size,max_gap", COMBOS, ids=COMBO_IDS)
def test_every_search_takes_the_same_samples(frames, culled_steps, size, max_gap):
    """(after the tests above, whose culled sample counts it compares: one rule, so one count per case whichever kernel casts it)"""
    names, _, _ = frames(size, max_gap)
    runs = culled_steps.get((size, max_gap), {})
    assert {"per_call", "batch_default", "batch_classic"} <= set(runs) and any(k.startswith("service_plain") for k in runs) and any(k.startswith("service_no_team_help") for k in runs), sorted(runs)
    first = runs["batch_default"]
    for k, v in runs.items():
        assert v == first, (k, [(n, a, b) for n, a, b in zip(names, v, first) if a != b])
