"""The crafted window-reuse cases (tests/window_reuse_cases.py; their expectations are asserted on the oracle by
tests/test_window_reuse_host.py) through k_lsd_service / k_lsd_service_c, byte-exact against the oracle -- lines, n_lines, rounds,
n_mask_px, and the sample count under exact statistics: a frame-granular pipeline of depth 3, plain, without team help, with help
first, and with the tile store capped at 4 tiles (every frame overflows it: the scan reads the mask in global memory, and reuses its
window under the same rule); 1024 x 768 (k_lsd_service, which keeps its window) and 2560 x 1440 (k_lsd_service_c, which does not)."""
import numpy as np
import pytest

import window_reuse_cases as WR

pytestmark = pytest.mark.gpu

SIZE_IDS = {WR.SIZES[0]: "768p", WR.SIZES[1]: "1440p"}
VARIANTS = ("plain", "no_team_help", "help_first", "tile_cap_4")


@pytest.fixture(scope="module")
def frames():
    """size -> ({name: Ref}, {name: frame on the device}); the oracle's answers once per session (window_reuse_cases.reference)."""
    import torch
    held = {}

    def get(size):
        if size not in held:
            held[size] = (WR.reference(size), {c.name: torch.from_numpy(WR.frame(c, *size)).cuda() for c in WR.cases()})
        return held[size]

    yield get
    held.clear()
    torch.cuda.empty_cache()


def _pipeline(vision, size, n, variant, **options):
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib
    lib = _lib.load()
    flags = {"no_team_help": _lib.PIPE_NO_TEAM_HELP, "help_first": _lib.PIPE_HELP_FIRST}.get(variant, 0)
    try:
        lib.smhv_debug_lsd_tile_cap(4 if variant == "tile_cap_4" else 0)      # (read when the pipeline is created)
        return smh.Pipeline(vision, size[0], size[1], n, 3, search="frame", flags=flags, **options)
    finally:
        lib.smhv_debug_lsd_tile_cap(0)


def _check(recs, refs, exact, tag):
    import squad_mortar_helper_amd as smh
    got = smh.results_to_dicts(recs)
    assert len(got) == len(refs)
    for i, (g, R) in enumerate(zip(got, refs)):
        name = R.case.name
        assert g["n_lines"] == len(R.lines) and np.array_equal(g["lines"], R.lines), (i, name, g["lines"], R.lines) + tag()
        assert g["rounds"] == R.rounds and g["n_mask_px"] == R.n_mask_px, (i, name, g["rounds"], R.rounds, g["n_mask_px"], R.n_mask_px) + tag()
        if exact:
            assert g["ray_steps"] == R.steps, (i, name, g["ray_steps"], R.steps) + tag()


def _run(pipe, d, refs, submissions, tag):
    import squad_mortar_helper_amd as smh
    for exact in (0, smh.STAGE_EXACT_STATS):
        slots = [pipe.submit(d.data_ptr(), len(refs), stages=smh.STAGE_MARKERS | exact, max_gap=WR.MAX_GAP) for _ in range(submissions)]
        pipe.wait()
        for s_ in sorted(set(slots)):
            _check(pipe.slots[s_].read_results(0, len(refs)), refs, exact, lambda: tag() + (bool(exact), s_))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("size", WR.SIZES, ids=SIZE_IDS.get)
def test_cases_through_the_service(vision, frames, size, variant):
    """a - d (and the frames of e and f, each on its own): every case in one submission, four submissions per statistics mode."""
    import torch
    refs, dev = frames(size)
    names = [c.name for c in WR.cases()]
    d = torch.stack([dev[n] for n in names])
    pipe = _pipeline(vision, size, len(names), variant)
    try:
        _run(pipe, d, [refs[n] for n in names], 4, lambda: (variant, pipe.search_stats()))
    finally:
        pipe.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_no_window_outlives_its_frame(vision, frames, variant):
    """e: 32 frames alternating two masks that differ only beyond the blob, eight submissions, the order swapped every time.  e_first_*: the
    blob is the frame's first candidate and lies inside the window the wave's last frame left (the host test shows it): a wave that kept
    its tag across frames would accept the blob alone or reject the continued one.  e_blob_*: the same behind a block of rejected
    candidates, where a helper that kept a window of another frame would."""
    import torch
    size = WR.SIZES[0]
    refs, dev = frames(size)
    pipe = _pipeline(vision, size, 32, variant)
    try:
        for pair in (("e_first_alone", "e_first_continued"), ("e_blob_alone", "e_blob_continued")):
            for k in range(8):
                names = [pair[(i + k) & 1] for i in range(32)]
                d = torch.stack([dev[n] for n in names])
                _run(pipe, d, [refs[n] for n in names], 1, lambda: (variant, pair, k, pipe.search_stats()))
    finally:
        pipe.close()


@pytest.mark.parametrize("variant", ("plain", "help_first"))
@pytest.mark.parametrize("size", WR.SIZES, ids=SIZE_IDS.get)
def test_helpers_keep_windows_of_their_own(vision, frames, size, variant):
    """f: one heavy frame (a few hundred rejected candidates in two bands, then three lines) among light ones: the desk engages, and with
    help first and a request after the first round the other workgroups' helpers too.  Records equal the oracle's, and the service's
    counters show that waves helped."""
    import torch
    refs, dev = frames(size)
    names = ["f_light"] * 7 + ["f_heavy"] + ["f_light"] * 8
    d = torch.stack([dev[n] for n in names])
    options = dict(remote_after=1, remote_tickets=4, remote_last=1) if variant == "help_first" else {}
    pipe = _pipeline(vision, size, len(names), variant, **options)
    try:
        _run(pipe, d, [refs[n] for n in names], 4, lambda: (variant, pipe.search_stats()))
        st = pipe.search_stats()
        print("search_stats:", st)
        assert st is not None and st["frames"] == 2 * 4 * len(names) and st["help_cycles_per_frame"] > 0, st
    finally:
        pipe.close()
