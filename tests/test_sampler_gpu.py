"""The cases of tests/sampler_cases.py (their expectations are asserted on the oracle by tests/test_sampler_host.py) through
k_lsd_service, whose rays take their first 64 steps through the service's own sampler (csrc/smh_lsd.hip, ray_batch<.., LEAN>): a
frame-granular pipeline at two depths (three and four slots) and once with the walk over the bit rows, byte for byte against the oracle -- lines, n_lines,
rounds and n_mask_px, and the sample count under exact statistics -- and every slot the same bytes."""
import numpy as np
import pytest

import sampler_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def groups():
    """[(max_gap, [Ref], frames on the device)]: the oracle's answers once per session, the frames uploaded once."""
    import torch
    ref = S.reference()
    held = [(gap, [ref[c.name] for c in cs], torch.from_numpy(np.stack([S.frame(c) for c in cs])).cuda()) for gap, cs in S.groups()]
    yield held
    held.clear()
    torch.cuda.empty_cache()


VARIANTS = (("depth_3", 3, 0), ("depth_4", 4, 0), ("walk_bit_rows", 3, "PIPE_WALK_BIT_ROWS"))      # (the frame-granular search starts at depth 3)


@pytest.mark.parametrize("variant,depth,flag", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_search_service(vision, groups, variant, depth, flag):
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import _lib
    pipe = smh.Pipeline(vision, S.SIZE[0], S.SIZE[1], max(len(refs) for _, refs, _ in groups), depth, search="frame", flags=getattr(_lib, flag) if flag else 0)
    try:
        for gap, refs, d in groups:
            n = len(refs)
            for exact in (0, smh.STAGE_EXACT_STATS):
                slots = [pipe.submit(d.data_ptr(), n, stages=smh.STAGE_MARKERS | exact, max_gap=gap) for _ in range(depth + 1)]
                pipe.wait()
                recs = {s_: pipe.slots[s_].read_results(0, n) for s_ in sorted(set(slots))}
                tag = lambda: (variant, gap, bool(exact), pipe.search_stats())          # the service's counters, on failure only
                for r in recs.values():
                    got = smh.results_to_dicts(r)
                    assert len(got) == n
                    for g, R in zip(got, refs):
                        name = R.case.name
                        assert g["n_lines"] == len(R.lines) and np.array_equal(g["lines"], R.lines), (name, g["lines"], R.lines) + tag()
                        assert g["rounds"] == R.rounds and g["n_mask_px"] == R.n_mask_px, (name, g["rounds"], R.rounds, g["n_mask_px"], R.n_mask_px) + tag()
                        if exact:
                            assert g["ray_steps"] == R.steps, (name, g["ray_steps"], R.steps) + tag()
                first = bytes(recs[slots[0]])
                assert all(bytes(r) == first for r in recs.values()), tag()
    finally:
        pipe.close()
