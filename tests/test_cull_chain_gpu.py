"""The crafted frames of the chained sector cull (tests/cull_chain_cases.py; the rule's soundness on their masks is asserted on the CPU by
tests/test_cull_chain_host.py) through every search -- k_lsd (the per-call trait path and the classic batch), k_lsd_tile (FrameBatch),
k_lsd_service (a frame-granular pipeline at 1024 x 768) and k_lsd_service_c (the same at 2560 x 1440): lines, n_lines, rounds and
n_mask_px byte for byte against the oracle; the sample count equal to the oracle's under exact statistics, and without them at most the
exact run's and the SAME in every search (they apply one rule, whichever the library was built with: the outer annulus alone, or with
-DSMH_CULL_CHAIN the chained one); for the blob with an arc 40 px away, which either rule casts little of, strictly below the exact run's.

  gaps      dotted bars with gaps of exactly T and T + 1 samples whose white samples fall at steps 18 / 19 and 34 / 35 from the first
            candidate (the ends of the middle window), along 0 degrees, the unit boundaries 6.4, 12.8, 83.2, 89.6 and 353.6 degrees, the
            wrap at 359.9 and the diagonal: the bars with gaps of T are found
  rejects   the blob with white in the outer annulus alone, and with white in both
  edges     candidates within 52 px of each image edge and corner, where the border cuts the annuli; bars that leave the image after
            50 and 51 steps"""
import numpy as np
import pytest

import cull_chain_cases as CC

pytestmark = pytest.mark.gpu

SIZE_IDS = {CC.SIZES[0]: "768p", CC.SIZES[1]: "1440p"}


@pytest.fixture(scope="module")
def frames():
    """size -> (names, [Ref], frames on the device); the oracle's answers once per session (cull_chain_cases.reference)."""
    import torch
    held = {}

    def get(size):
        if size not in held:
            refs = CC.reference(size)
            names = [c.name for c in CC.cases()]
            held[size] = (names, [refs[n] for n in names], torch.from_numpy(np.stack([CC.frame(c, *size) for c in CC.cases()])).cuda())
        return held[size]

    yield get
    held.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def culled_steps():
    """size -> {search: [ray_steps per case]} of the culled runs, filled by the tests below and compared by the last one."""
    return {}


def _check(got, refs, exact, tag):
    assert len(got) == len(refs)
    for g, R in zip(got, refs):
        name = R.case.name
        assert g["n_lines"] == len(R.lines) and np.array_equal(g["lines"], R.lines), (name, g["lines"], R.lines) + tag
        assert g["rounds"] == R.rounds and g["n_mask_px"] == R.n_mask_px, (name, g["rounds"], R.rounds, g["n_mask_px"], R.n_mask_px) + tag
        if exact:
            assert g["ray_steps"] == R.steps, (name, g["ray_steps"], R.steps) + tag
        else:
            assert g["ray_steps"] <= R.steps, (name, g["ray_steps"], R.steps) + tag
            if name == "arc_outer_only":
                assert g["ray_steps"] < R.steps, (name, g["ray_steps"], R.steps) + tag


@pytest.mark.parametrize("size", CC.SIZES, ids=SIZE_IDS.get)
def test_per_call_trait_path(vision, frames, culled_steps, size):
    import squad_mortar_helper_amd as smh
    names, refs, d = frames(size)
    steps = []
    st = smh.VisionState(grayscale_map=True, max_gap=CC.MAX_GAP)
    try:
        for i, R in enumerate(refs):
            res = st.process(vision, d[i].cpu().numpy())
            assert np.array_equal(vision.lsd_image(), R.mask), names[i]
            assert res.markers.shape == R.lines.shape and np.array_equal(res.markers, R.lines), (names[i], res.markers, R.lines)
            r_fast, s_fast = vision.lsd_stats(CC.MAX_GAP, exact=False)
            r_exact, s_exact = vision.lsd_stats(CC.MAX_GAP, exact=True)
            assert r_fast == r_exact == R.rounds and s_exact == R.steps and s_fast <= s_exact, (names[i], r_fast, r_exact, R.rounds, s_fast, s_exact, R.steps)
            if names[i] == "arc_outer_only":
                assert s_fast < s_exact, (s_fast, s_exact)
            steps.append(s_fast)
    finally:
        st.close()
    culled_steps.setdefault(size, {})["per_call"] = steps


@pytest.mark.parametrize("variant", ("default", "classic"))
@pytest.mark.parametrize("size", CC.SIZES, ids=SIZE_IDS.get)
def test_frame_batch(vision, frames, culled_steps, size, variant):
    import torch
    import squad_mortar_helper_amd as smh
    lib = smh._lib.load()
    names, refs, d = frames(size)
    fb = smh.FrameBatch(vision, size[0], size[1], len(refs))
    try:
        lib.smhv_debug_lsd_classic(int(variant == "classic"))
        for exact in (0, smh.STAGE_EXACT_STATS):
            fb.run(d.data_ptr(), len(refs), stages=smh.STAGE_MARKERS | exact, max_gap=CC.MAX_GAP, stream=torch.cuda.current_stream().cuda_stream)
            got = smh.results_to_dicts(fb.read_results(0, len(refs)))
            _check(got, refs, exact, (variant, bool(exact)))
            if not exact:
                culled_steps.setdefault(size, {})["batch_" + variant] = [g["ray_steps"] for g in got]
    finally:
        lib.smhv_debug_lsd_classic(0)
        fb.close()


@pytest.mark.parametrize("variant", ("plain", "no_team_help"))
@pytest.mark.parametrize("size", CC.SIZES, ids=SIZE_IDS.get)
def test_search_service(vision, frames, culled_steps, size, variant):
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib
    names, refs, d = frames(size)
    pipe = smh.Pipeline(vision, size[0], size[1], len(refs), 3, search="frame", flags=_lib.PIPE_NO_TEAM_HELP if variant == "no_team_help" else 0)
    try:
        assert pipe.peek()["service_workgroups"] > 0
        for exact in (0, smh.STAGE_EXACT_STATS):
            slots = [pipe.submit(d.data_ptr(), len(refs), stages=smh.STAGE_MARKERS | exact, max_gap=CC.MAX_GAP) for _ in range(3)]
            pipe.wait()
            for s_ in sorted(set(slots)):
                got = smh.results_to_dicts(pipe.slots[s_].read_results(0, len(refs)))
                _check(got, refs, exact, (variant, bool(exact), s_))
                if not exact:
                    culled_steps.setdefault(size, {})["service_%s_%d" % (variant, s_)] = [g["ray_steps"] for g in got]
    finally:
        pipe.close()


@pytest.mark.parametrize("size", CC.SIZES, ids=SIZE_IDS.get)
def test_every_search_takes_the_same_samples(frames, culled_steps, size):
    """(after the tests above, whose culled sample counts it compares: one rule, so one count per case whichever kernel casts it)"""
    names, _, _ = frames(size)
    runs = culled_steps.get(size, {})
    assert {"per_call", "batch_default", "batch_classic"} <= set(runs) and any(k.startswith("service_") for k in runs), sorted(runs)
    first = runs["batch_default"]
    for k, v in runs.items():
        assert v == first, (k, [(n, a, b) for n, a, b in zip(names, v, first) if a != b])
