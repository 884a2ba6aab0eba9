"""Pipelines whose submissions vary in size (tests/pipeline_size_cases.py): a slot runs M frames, then 1, then M - 1 with other
content.  After wait(slot), with the later submissions still in flight: records 0 .. n - 1 are byte-equal to a plain
FrameBatch.run of the same n frames and match the oracle; records n .. are, byte for byte, what the slot held there before (the
rule stated at smhv_batch_run in include/smh_vision_hip.h) and the oracle's for the frame the slot model names; the ui_map, the
lazy mask and the tile-major mask at indices 0, n - 1, n and the slot's high-water mark - 1 are the oracle's for the frame the
model names (a closed frame keeps its older images).  Then the adaptive pipeline on such submissions, and ingest queues whose
slabs go straight into Pipeline.submit.  Every comparison is exact; tests/test_pipeline_sizes_host.py pins the expectations."""
import zlib

import numpy as np
import pytest

import geometry_sweep_cases as G
import pipeline_size_cases as P
from tile_mask_check import check_tile_mask

pytestmark = pytest.mark.gpu


class World:
    """One size on the device: the K frames with period K in one buffer of M + K frames (a rotation is a pointer offset), the
    oracle's outputs, and the plain runs -- one FrameBatch.run per distinct (n, rotation), computed once and shared."""

    def __init__(self, vision, s):
        import torch
        import squad_mortar_helper_amd as smh
        self.vision, self.s = vision, s
        self.frames, self.infos, self.refs = P.oracle_of(s)
        self.open_of = [bool(r["map_open"]) for r in self.refs]
        self.fbytes = s.W * s.H * 4
        d = torch.from_numpy(self.frames).cuda()
        self.buf = d.repeat(-(-(s.M + P.K) // P.K), 1, 1, 1)[:s.M + P.K].contiguous()
        del d
        torch.cuda.synchronize()
        self.per = [(i["scales_start_y"], i["anchors"]) for i in self.infos]
        self._plain = {}
        self._fb = smh.FrameBatch(vision, s.W, s.H, s.M)
        self.plain_runs = 0

    def ptr(self, rot):
        return self.buf.data_ptr() + rot * self.fbytes

    def anchors(self, n, rot):
        import squad_mortar_helper_amd as smh
        return smh.make_anchors([self.per[P.frame_of(i, rot)] for i in range(n)])

    def plain(self, n, rot):
        """Record bytes [n] of a plain FrameBatch.run over the n frames of (n, rot), each held to the oracle once."""
        import torch
        import squad_mortar_helper_amd as smh
        from test_geometry_sweep_gpu import _check_record
        if (n, rot) not in self._plain:
            self._fb.run(self.ptr(rot), n, stages=smh.STAGE_ALL, max_gap=G.MAX_GAP, anchors=self.anchors(n, rot), stream=torch.cuda.current_stream().cuda_stream)
            recs = self._fb.read_results(0, n)
            for i, r in enumerate(smh.results_to_dicts(recs)):
                f = P.frame_of(i, rot)
                _check_record(r, self.refs[f], self.infos[f], smh.STAGE_ALL, ("plain", n, rot, i))
            self._plain[(n, rot)] = [bytes(r) for r in recs]
            self.plain_runs += 1
        return self._plain[(n, rot)]

    def close(self):
        import torch
        self._fb.close()
        self.buf = None
        torch.cuda.empty_cache()


@pytest.fixture(scope="module", params=P.SIZES, ids=P.SIZE_IDS)
def world(request, vision):
    w = World(vision, request.param)
    yield w
    w.close()


class SlotCheck:
    """The true slot model of one slot, what the slot's records were when they were last read, and the checks of one submission."""

    def __init__(self, world, M):
        self.w, self.M = world, M
        self.model = P.SlotModel(M, world.open_of)
        self.held = [None] * M                                       # (record bytes as last read; None: not read yet)

    def submitted(self, n, rot):
        self.model.submit(n, rot)

    def check(self, fb, n, rot, ctx, images=True, tiles_fused=None, tiles_may_skip=False):
        import squad_mortar_helper_amd as smh
        from test_geometry_sweep_gpu import _check_record
        w, M, model = self.w, self.M, self.model
        L = smh._lib
        recs = fb.read_results(0, M, check=True)                     # (raises if the library gave a frame up)
        raw = [bytes(r) for r in recs]
        assert raw[:n] == w.plain(n, rot), (ctx, [i for i in range(n) if raw[i] != w.plain(n, rot)[i]])
        dicts = smh.results_to_dicts(recs)
        for i in range(M):
            f = model.rec[i]
            if f is None:
                assert not any(raw[i]), (ctx, i, "a record nothing wrote")
                continue
            _check_record(dicts[i], w.refs[f], w.infos[f], smh.STAGE_ALL, (ctx, i, f))
            if i >= n:
                assert raw[i] == self.held[i], (ctx, i, "a record beyond n changed")
        self.held = raw
        if not images:
            return
        for i in model.image_indices(n):
            if model.img[i] is None:
                continue
            f, n_w = model.img[i]
            ref = w.refs[f]
            assert np.array_equal(fb.read_image(L.IMAGE_UI_MAP, i), ref["ui_map"]), (ctx, i, f, "ui_map")
            assert np.array_equal(fb.read_image(L.VIEW_LSD_INPUT, i), ref["lsd"]), (ctx, i, f, "mask")
            written = fb.tile_mask(i)[0] is not None
            f_c, n_c = model.cover[i]                                # the flag follows the newest submission that COVERED the index
            if not w.open_of[f_c]:
                assert not written, (ctx, i, f_c, "a closed frame reads as bit rows only")
            elif tiles_fused is not None and tiles_may_skip:         # the grid-stride form never writes it; the other form by the band rule
                assert not written or P.band_rows(w.s, n_c, tiles_fused)[1], (ctx, i, f_c, n_c, written)
            elif tiles_fused is not None:                            # the band rule alone decides
                assert written == P.band_rows(w.s, n_c, tiles_fused)[1], (ctx, i, f_c, n_c, written)
            check_tile_mask(fb, i, ref["lsd"], written, (ctx, i, f))


def _drive(world, pipe, depth, seq, ctx, tiles_fused=None, images_every=1, after_submit=None, tiles_may_skip=False):
    """Submit seq; check every submission after wait(slot) once depth - 1 later ones are in flight.  -> submissions checked."""
    import squad_mortar_helper_amd as smh
    s = world.s
    checks = [SlotCheck(world, s.M) for _ in range(depth)]
    inflight, done = [], 0

    def check_oldest():
        nonlocal done
        slot, n, rot, j = inflight.pop(0)
        pipe.wait(slot)
        checks[slot].check(pipe.slots[slot], n, rot, (ctx, j, slot, n, rot), images=(j % images_every == 0), tiles_fused=tiles_fused, tiles_may_skip=tiles_may_skip)
        done += 1
    keep = []
    for j, (n, rot) in enumerate(seq):
        a = world.anchors(n, rot)
        keep.append(a)
        slot = pipe.submit(world.ptr(rot), n, stages=smh.STAGE_ALL, max_gap=G.MAX_GAP, anchors=a)
        assert slot == j % depth
        if after_submit:
            after_submit(j, slot, n)
        # the model of a slot moves on when its submission is CHECKED (the slot is not reused before: at most depth in flight)
        inflight.append((slot, n, rot, j))
        if len(inflight) == depth:
            s_, n_, r_, _ = inflight[0]
            checks[s_].submitted(n_, r_)
            check_oldest()
    while inflight:
        s_, n_, r_, _ = inflight[0]
        checks[s_].submitted(n_, r_)
        check_oldest()
    return done


SCHEDULES = [("batch", 2, 0), ("batch", 4, 0), ("frame", 3, 0), ("frame", 4, 0), ("frame", 3, "PIPE_WALK_BIT_ROWS"), ("frame", 4, "PIPE_WALK_BIT_ROWS"),
             ("frame", 3, "PIPE_NO_TEAM_HELP"), ("frame", 4, "PIPE_NO_TEAM_HELP")]


@pytest.mark.parametrize("search,depth,flag", SCHEDULES, ids=["%s-d%d%s" % (s_, d, "-" + f[5:].lower() if f else "") for s_, d, f in SCHEDULES])
def test_slots_take_submissions_of_varying_size(vision, world, search, depth, flag):
    """4 x depth submissions per schedule (n cycling through M, 1, M - 1 and two sizes with other band heights, every one another
    rotation of six frames, two of them closed), each checked as the module's text says.
    The tile-major mask's `written` flag of an open frame is held to the band rule of the submission that covered it wherever the
    rule alone decides: a frame-granular pipeline (its passes run beside the service; SMHV_PIPE_WALK_BIT_ROWS and
    SMHV_PIPE_NO_TEAM_HELP change the search's side only) and a batch-granular one below depth 3 (a pass that runs alone).  From
    depth 3 on a batch-granular pipeline switches its capped, grid-stride form of the pass on and off by what it measures; that
    form never writes the mask and the other follows the rule beside other kernels, so there the flag may be 0 at any n and may be
    1 only where that rule says so."""
    import squad_mortar_helper_amd as smh
    s = world.s
    seq = P.sequence(s, depth)
    P.check_sequence(s, depth, world.refs, seq)
    fused, may_skip = (2, False) if search == "frame" else (1, False) if depth < 3 else (2, True)
    pipe = smh.Pipeline(vision, s.W, s.H, s.M, depth, search=search, flags=getattr(smh._lib, flag) if flag else 0)
    try:
        assert _drive(world, pipe, depth, seq, (search, depth, flag), tiles_fused=fused, tiles_may_skip=may_skip) == len(seq) == P.USES * depth
        pipe.wait()
    finally:
        pipe.close()


def test_adaptive_pipeline_on_submissions_of_varying_size(vision):
    """Depth 6, 568 x 361, 24 frames.  Phase 1: 208 submissions with n cycling through 20..24 -- one workload for the mode
    controller -- every record checked, images at every 16th; afterwards the pipeline has settled, and submissions of both searches
    went through every slot with different n.  Phase 2: 25 submissions alternating 24 with 3, 5, 7, ...: every record right."""
    import squad_mortar_helper_amd as smh
    s, depth = P.ADAPTIVE, 6
    settle = 26 * depth + 52
    P.check_adaptive_sequence(depth, settle)
    seq, _ = P.adaptive_sequence(depth, settle)
    world = World(vision, s)
    pipe = smh.Pipeline(vision, s.W, s.H, s.M, depth)
    try:
        st0 = pipe.search_stats()
        assert st0["adaptive"] and not st0["settled"]
        took = []                                                    # (slot, n, True where the search service took the submission)
        seen = [pipe.peek()["last_seq"]]
        after = {}

        def note(j, slot, n):
            now = pipe.peek()["last_seq"]                            # (the service's own count of submissions: no device-wide wait)
            took.append((slot, n, now != seen[0]))
            seen[0] = now
            if j == settle - 1:                                      # phase 1 is over; the pipeline goes on running into phase 2
                after["stats"] = pipe.search_stats()
        assert _drive(world, pipe, depth, seq, "adaptive", images_every=16, after_submit=note) == len(seq) == settle + 4 * depth + 1
        st = after["stats"]
        assert st["settled"] and min(st["measured_frames_per_s"].values()) > 0, st
        for slot in range(depth):
            for kind in (True, False):
                assert len({n for s_, n, k in took[:settle] if s_ == slot and k == kind}) >= 2, (slot, kind)
        pipe.wait()
        assert pipe.search_stats()["adaptive"]
    finally:
        pipe.close()
        world.close()


@pytest.mark.parametrize("roi_upload", [False, True], ids=["plain-queue", "roi-upload-queue"])
def test_ingest_slabs_of_varying_size_go_straight_into_the_pipelines(vision, roi_upload):
    """A queue of capacity 24 takes four capture sequences whose duplicates leave slabs of 1, 6, 24 and 2 frames; batch()'s pointer
    goes into Pipeline.submit of a frame-granular and a batch-granular pipeline, wait(slot) before reset(); every slab's records
    are the oracle's for the frames the reference's duplicate rule keeps, in both pipelines."""
    import squad_mortar_helper_amd as smh
    from squad_mortar_helper_amd import ingest
    from test_geometry_sweep_gpu import _check_record
    s = P.ADAPTIVE
    frames, infos, refs = P.oracle_of(s)
    crcs = [zlib.crc32(f.tobytes()) for f in frames]
    from oracle import oracle as o
    kept = P.check_capture_slabs(s.M, crcs, o.capture_dedupe)
    q = smh.IngestQueue(vision, s.W, s.H, slots=4, capacity=s.M, roi_upload=roi_upload)
    pipes = [smh.Pipeline(vision, s.W, s.H, s.M, 3, search="frame"), smh.Pipeline(vision, s.W, s.H, s.M, 2, search="batch")]
    try:
        k = new = dup = 0
        for caps, want in zip(P.capture_slabs(s.M), kept):
            for i in caps:
                if k % 2:
                    q.push(frames[i])
                else:
                    q.acquire()[...] = frames[i]
                    q.commit()
                k += 1
            ptr, n, crc = q.batch()
            new, dup = new + len(want), dup + len(caps) - len(want)
            assert n == len(want) and crc == crcs[want[-1]] and q.counts() == (new, dup)
            anchors = smh.make_anchors([(infos[f]["scales_start_y"], infos[f]["anchors"]) for f in want])
            slots = [p.submit(ptr, n, stages=smh.STAGE_ALL, max_gap=G.MAX_GAP, anchors=anchors) for p in pipes]
            out = []
            for p, slot in zip(pipes, slots):
                p.wait(slot)                                         # the slab is read until here: reset() comes after
                recs = p.slots[slot].read_results(0, n, check=True)
                out.append([bytes(r) for r in recs])
                for i, r in enumerate(smh.results_to_dicts(recs)):
                    _check_record(r, refs[want[i]], infos[want[i]], smh.STAGE_ALL, (roi_upload, len(want), i))
            assert out[0] == out[1]
            q.reset()
        assert ingest.crc32_host(frames[kept[-1][-1]]) == q.batch()[2]
    finally:
        for p in pipes:
            p.close()
        q.close()
