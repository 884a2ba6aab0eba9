// smh_feedtiles.inc -- the remote-viewer feed's map tiles: public entry points (smh_vision_hip.h, "remote-viewer feed: map tiles";
// the rule in smh_maptiles.h, device code in smh_feedtiles.hip).  Included behind smh_feed.inc at the end of smh_runtime.cpp.

// The feed's tile memory, made by the first tile call, all or nothing; the tile bitmaps again when a call needs more words than
// any before it (the kernels of the feed's previous call may still read the old ones: the host waits for it first).
static int feed_tiles_memory(smhv_feed *f, uint32_t n, uint32_t words) {
	const bool first_call = !f->d_kept;
	if (first_call) {
		const size_t frames = f->max_frames;
		struct { void **slot; size_t bytes; bool zero; } parts[] = {
			{(void **)&f->d_kept, (size_t)((f->capacity + 15ull) & ~15ull), false}, {(void **)&f->d_kstate, sizeof(uint32_t) * 4u, true},
			{(void **)&f->d_tctl, sizeof(uint32_t) * 4u, true},                      {(void **)&f->d_tbase, sizeof(uint32_t) * frames, false},
			{(void **)&f->d_tinfo, sizeof(uint32_t) * 2u * frames, false},           {(void **)&f->d_titems, sizeof(FeedTileItem) * frames, false}};
		hipError_t e = hipSuccess;
		for (auto &p : parts) {
			if (e == hipSuccess) e = hipMalloc(p.slot, p.bytes);
			if (e == hipSuccess && p.zero) e = hipMemset(*p.slot, 0, p.bytes);
		}
		if (e != hipSuccess) {
			for (auto &p : parts) {
				if (*p.slot) (void)hipFree(*p.slot);
				*p.slot = nullptr;
			}
			return fail(SMHV_E_HIP, "feed tiles: the kept map and the tile lists (%llu bytes, %u frames): %s", (unsigned long long)f->capacity, f->max_frames, hipGetErrorString(e));
		}
	}
	const size_t need = (size_t)n * words;
	if (f->tbits_words < need) {
		uint2 *fresh = nullptr;
		const hipError_t e = hipMalloc((void **)&fresh, sizeof(uint2) * need);
		if (e != hipSuccess) {
			if (first_call) {                                     // all or nothing: a failed first call leaves the feed without tile memory
				void **made[] = {(void **)&f->d_kept, (void **)&f->d_kstate, (void **)&f->d_tctl, (void **)&f->d_tbase, (void **)&f->d_tinfo, (void **)&f->d_titems};
				for (void **p : made) { (void)hipFree(*p); *p = nullptr; }
			}
			return fail(SMHV_E_HIP, "feed tiles: the tile bitmaps (%u frames of %u words): %s", n, words, hipGetErrorString(e));
		}
		if (f->d_tbits) {
			if (f->used) {
				const hipError_t w = wait_event(f->ev_last);
				if (w != hipSuccess) { (void)hipFree(fresh); HIPCHK(w); }
			}
			(void)hipFree(f->d_tbits);
		}
		f->d_tbits = fresh; f->tbits_words = need;
	}
	return SMHV_OK;
}

// flags: none is defined for a tile call, and a snapshot has no base
static int feed_tiles_flags(uint32_t flags, const char *what) {
	if (flags & ~SMHV_FEED_SNAPSHOT) return fail(SMHV_E_INVALID, "%s: unknown feed flags 0x%x", what, flags);
	if (flags) return fail(SMHV_E_INVALID, "%s: SMHV_FEED_SNAPSHOT with map tiles (a snapshot has no base: use the call without tiles)", what);
	return SMHV_OK;
}

// The tile call's kernels on `s`, behind the feed's previous call (after feed_check and feed_tiles_flags).
static int feed_enqueue_tiles(smhv_feed *f, const FeedSrc &v, const smhv_frame_result *res, uint32_t first, uint32_t n, hipStream_t s) {
	const TileGrid g = tile_grid(v.w, v.h);
	const uint32_t words = (tile_count(g) + 31u) / 32u;
	int rc = feed_tiles_memory(f, n, words);
	if (rc) return rc;
	FeedTilesRun t;
	memset(&t, 0, sizeof t);
	rc = feed_prepare(f, v, res, first, n, 0u, s, &t.r);
	if (rc) return rc;
	t.kept = f->d_kept; t.kstate = f->d_kstate; t.ctl = f->d_tctl; t.base = f->d_tbase; t.info = f->d_tinfo;
	t.bits = f->d_tbits; t.items = f->d_titems; t.words = words;
	HIPCHK(launch_feed_tiles(t, s));
	HIPCHK(hipEventRecord(f->ev_last, s));
	f->used = true;
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_batch_feed_tiles(smhv_batch *b, smhv_feed *f, uint32_t first, uint32_t n, uint32_t flags, void *stream) {
	if (!b || !f) return fail(SMHV_E_INVALID, "batch_feed: null argument");
	CTX_OPEN(b->ctx);
	CTX_OPEN(f->ctx);
	int rc = check_device(f->ctx->device, b->ctx->device, "batch_feed", "feed", "batch");
	if (rc) return rc;
	rc = check_frames(b, first, n, "batch_feed");
	if (rc) return rc;
	FeedSrc v;
	rc = feed_batch_source(b, first, (uint32_t)SMHV_VIEW_NONE, false, &v);
	if (rc) return rc;
	rc = feed_tiles_flags(flags, "batch_feed");
	if (rc) return rc;
	rc = feed_check(f, v.w, v.h, n, flags, "batch_feed");
	if (rc) return rc;
	rc = feed_batch_source(b, first, (uint32_t)SMHV_VIEW_NONE, true, &v);
	if (rc) return rc;
	HIPCHK(hipSetDevice(b->ctx->device));
	rc = batch_materialize_ui(b, (hipStream_t)stream);          // (a grey batch owes the RGBA ui slab until it is read)
	if (rc) return rc;
	return feed_enqueue_tiles(f, v, b->d_results + first, first, n, (hipStream_t)stream);
}

extern "C" SMHV_API int smhv_feed_frame_tiles(smhv_ctx *c, smhv_feed *f, const smhv_line *lines, uint32_t n_lines, const double *mpx, const uint32_t minimap[4],
                                              uint32_t flags) {
	int rc = require_open(c, "feed_frame");
	if (rc) return rc;
	CTX_OPEN(c);
	if (!f || (n_lines && !lines)) return fail(SMHV_E_INVALID, "feed_frame: null argument");
	CTX_OPEN(f->ctx);
	rc = check_device(f->ctx->device, c->device, "feed_frame", "feed", "context");
	if (rc) return rc;
	if (n_lines > SMHV_MAX_LINES) return fail(SMHV_E_INVALID, "feed_frame: %u lines (at most %u)", n_lines, (unsigned)SMHV_MAX_LINES);
	rc = feed_tiles_flags(flags, "feed_frame");
	if (rc) return rc;
	smhv_batch *b = c->fb;
	const FeedSrc v = feed_src_ui(b->g, b->d_ui);
	rc = feed_check(f, v.w, v.h, 1, flags, "feed_frame");
	if (rc) return rc;
	HIPCHK(hipSetDevice(c->device));
	rc = batch_materialize_ui(b, c->s_main);                   // (the single-frame batch's pass writes RGBA: nothing is ever owed)
	if (rc) return rc;
	if (f->used) HIPCHK(wait_event(f->ev_last));              // (the staging record: the previous call's upload has left it)
	rc = feed_tiles_memory(f, 1u, (tile_count(tile_grid(v.w, v.h)) + 31u) / 32u);
	if (rc) return rc;
	smhv_frame_result *h = f->h_rec;
	memset(h, 0, sizeof *h);
	h->map_open = 1u; h->status = SMHV_FRAME_OK;
	h->n_lines = n_lines;
	if (n_lines) memcpy(h->lines, lines, sizeof(smhv_line) * n_lines);
	if (mpx) { h->mpx = *mpx; h->has_mpx = 1u; }
	if (minimap) { memcpy(h->minimap, minimap, sizeof h->minimap); h->has_minimap = 1u; }
	HIPCHK(hipMemcpyAsync(f->d_rec, h, sizeof *h, hipMemcpyHostToDevice, c->s_main));
	return feed_enqueue_tiles(f, v, f->d_rec, 0, 1, c->s_main);
}
