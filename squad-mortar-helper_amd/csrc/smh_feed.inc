// smh_feed.inc -- the remote-viewer feed: public entry points (smh_vision_hip.h; device code in smh_feed.hip) and the host-only
// rest of the web server's protocol (web/src/lib.rs:37-214).  Included at the end of smh_runtime.cpp.

struct smhv_feed {
	smhv_ctx *ctx = nullptr;
	uint64_t capacity = 0;
	uint32_t max_frames = 0;
	uint8_t *d_bytes = nullptr;
	smhv_feed_header *d_header = nullptr;
	smhv_feed_entry *d_entries = nullptr;
	uint32_t *d_state = nullptr, *d_raw = nullptr, *d_tab = nullptr;
	FeedMap *d_maps = nullptr;
	uint32_t tab_w = 0, tab_h = 0, tab_xoff = 0, tab_ppg = 0; // the message geometry d_tab was built for (k_feed_tables / k_feed_view_tables)
	uint8_t *d_view = nullptr;                                // smhv_feed_frame_view: the materialised view behind its lead-in of zeros
	size_t view_cap = 0;
	hipEvent_t ev_last = nullptr;                             // the feed's most recent call: the next one is ordered behind it
	bool used = false;
	smhv_frame_result *d_rec = nullptr, *h_rec = nullptr;     // smhv_feed_frame: the call's record (device, pinned staging)
	// map tiles (smh_feedtiles.inc), made by the first tile call: the kept map (room for any map the feed accepts), its state,
	// the plan's words for the copies, per frame the base, the sums and the MapTiles items; the tile bitmaps grow with the geometry
	uint8_t *d_kept = nullptr;
	uint32_t *d_kstate = nullptr, *d_tctl = nullptr, *d_tbase = nullptr, *d_tinfo = nullptr;
	FeedTileItem *d_titems = nullptr;
	uint2 *d_tbits = nullptr;
	size_t tbits_words = 0;
};

extern "C" SMHV_API void smhv_feed_destroy(smhv_feed *f) {
	if (!f) return;
	if (f->ctx) (void)hipSetDevice(f->ctx->device);
	(void)hipDeviceSynchronize();
	void *ptrs[] = {f->d_bytes, f->d_header, f->d_entries, f->d_state, f->d_raw, f->d_tab, f->d_maps, f->d_rec, f->d_view, f->d_kept, f->d_kstate, f->d_tctl, f->d_tbase, f->d_tinfo, f->d_titems, f->d_tbits};
	for (void *p : ptrs)
		if (p) (void)hipFree(p);
	if (f->h_rec) (void)hipHostFree(f->h_rec);
	if (f->ev_last) (void)hipEventDestroy(f->ev_last);
	ctx_release(f->ctx);
	delete f;
}

extern "C" SMHV_API int smhv_feed_create(smhv_ctx *c, uint64_t capacity_bytes, uint32_t max_frames, smhv_feed **out) {
	if (!c || !out) return fail(SMHV_E_INVALID, "feed_create: null argument");
	*out = nullptr;
	CTX_OPEN(c);
	if (max_frames == 0u || max_frames > 65535u) return fail(SMHV_E_INVALID, "feed_create: max_frames %u (1 .. 65535)", max_frames);
	if (capacity_bytes < 16u) return fail(SMHV_E_INVALID, "feed_create: a capacity of %llu bytes", (unsigned long long)capacity_bytes);
	HIPCHK(hipSetDevice(c->device));
	smhv_feed *f = new (std::nothrow) smhv_feed();
	if (!f) return fail(SMHV_E_INVALID, "out of host memory");
	c->refs.fetch_add(1, std::memory_order_relaxed);
	f->ctx = c; f->capacity = capacity_bytes; f->max_frames = max_frames;
	const size_t n = max_frames;
	hipError_t e = hipMalloc((void **)&f->d_bytes, (size_t)capacity_bytes);
	if (e == hipSuccess) e = hipMalloc((void **)&f->d_header, sizeof(smhv_feed_header));
	if (e == hipSuccess) e = hipMemset(f->d_header, 0, sizeof(smhv_feed_header));
	if (e == hipSuccess) e = hipMalloc((void **)&f->d_entries, sizeof(smhv_feed_entry) * 3u * n);
	if (e == hipSuccess) e = hipMalloc((void **)&f->d_state, sizeof(uint32_t) * 2u);
	if (e == hipSuccess) e = hipMemset(f->d_state, 0, sizeof(uint32_t) * 2u);
	if (e == hipSuccess) e = hipMalloc((void **)&f->d_raw, sizeof(uint32_t) * n);
	if (e == hipSuccess) e = hipMalloc((void **)&f->d_tab, sizeof(uint32_t) * (1024u + SMH_FEED_MAX_ROWS));
	if (e == hipSuccess) e = hipMalloc((void **)&f->d_maps, sizeof(FeedMap) * n);
	if (e == hipSuccess) e = hipMalloc((void **)&f->d_rec, sizeof(smhv_frame_result));
	if (e == hipSuccess) e = hipHostMalloc((void **)&f->h_rec, sizeof(smhv_frame_result), hipHostMallocDefault);
	if (e == hipSuccess) e = hipEventCreateWithFlags(&f->ev_last, hipEventDisableTiming);
	if (e != hipSuccess) { smhv_feed_destroy(f); return fail(SMHV_E_HIP, "feed_create (%llu bytes, %u frames): %s", (unsigned long long)capacity_bytes, max_frames, hipGetErrorString(e)); }
	*out = f;
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_feed_reset(smhv_feed *f) {
	if (!f) return fail(SMHV_E_INVALID, "feed_reset: null feed");
	CTX_OPEN(f->ctx);
	HIPCHK(hipSetDevice(f->ctx->device));
	if (f->used) HIPCHK(wait_event(f->ev_last));
	HIPCHK(hipMemset(f->d_state, 0, sizeof(uint32_t) * 2u));
	return SMHV_OK;
}

// What a call hashes and sends as the Map: the message's size and where its bytes come from.  mode SMH_RND_SRC_UI: the ui_map as
// it lies in the ui slab; SMH_RND_SRC_GRAY / PREPROCESS / CROPPED: a debug view generated from a slab (launch_feed_view);
// SMH_RND_SRC_RGBA: one tight image at `base` behind `lead` zero dwords (launch_feed_image).
struct FeedSrc {
	const uint8_t *base = nullptr;                            // at the call's first frame
	uint64_t pitch = 0, stride = 0;
	uint32_t w = 0, h = 0, xoff = 0, quads = 0, ppg = 4, mode = SMH_RND_SRC_UI;
	uint32_t lead = 0;
};

// one frame's worst case in the buffer: the first message at 6, UpdateState with bounds, a Map of w x h, 32 marker lines
static uint64_t feed_worst_case(uint32_t w, uint32_t h) {
	const uint64_t map_len = 10ull + (uint64_t)w * h * 4u;
	return 6ull + 32ull + ((map_len + 15ull) & ~15ull) + 7ull + 16ull * SMHV_MAX_LINES;
}

// what a call can get wrong without the device being asked; w x h: the Map of the call's source
static int feed_check(const smhv_feed *f, uint32_t w, uint32_t h, uint32_t n, uint32_t flags, const char *what) {
	if (flags & ~SMHV_FEED_SNAPSHOT) return fail(SMHV_E_INVALID, "%s: unknown feed flags 0x%x", what, flags);
	if (n == 0u || n > f->max_frames) return fail(SMHV_E_INVALID, "%s: %u frames in one call of a feed of %u", what, n, f->max_frames);
	if (f->capacity < feed_worst_case(w, h))
		return fail(SMHV_E_INVALID, "%s: the feed's %llu bytes are below one frame's worst case at a %u x %u map (%llu)", what, (unsigned long long)f->capacity, w, h,
		            (unsigned long long)feed_worst_case(w, h));
	if (h > SMH_FEED_MAX_ROWS) return fail(SMHV_E_INVALID, "%s: a map of %u rows (at most %u)", what, h, SMH_FEED_MAX_ROWS);
	return SMHV_OK;
}

static FeedSrc feed_src_ui(const Geom &g, const uint8_t *ui) {
	FeedSrc v;
	v.base = ui; v.pitch = g.ui_pitch; v.stride = g.ui_stride;
	v.w = g.rw; v.h = g.rh; v.xoff = g.m_xoff; v.quads = g.m_quads;
	return v;
}

// `s` behind the feed's previous call, the CRC's tables for the call's source, and the call's FeedRun (after feed_check).
// v / res: the call's first frame.
static int feed_prepare(smhv_feed *f, const FeedSrc &v, const smhv_frame_result *res, uint32_t first, uint32_t n, uint32_t flags, hipStream_t s, FeedRun *out) {
	if (f->used) HIPCHK(hipStreamWaitEvent(s, f->ev_last, 0));
	const bool image = v.mode == SMH_RND_SRC_RGBA;
	// the CRC's description of the message: an image is rows of SMH_FEED_IMAGE_ROW dwords, its lead-in of zeros included
	const uint32_t cw = image ? SMH_FEED_IMAGE_ROW : v.w, ch = image ? (uint32_t)(((uint64_t)v.w * v.h + v.lead) / SMH_FEED_IMAGE_ROW) : v.h;
	const uint32_t cquads = image ? SMH_FEED_IMAGE_ROW / 4u : v.quads, cxoff = image ? 0u : v.xoff;
	if (f->tab_w != cw || f->tab_h != ch || f->tab_xoff != cxoff || f->tab_ppg != v.ppg) {
		if (v.ppg == 4u) HIPCHK(launch_feed_tables(f->d_tab, cw, ch, cxoff, cquads, s));
		else HIPCHK(launch_feed_view_tables(f->d_tab, cw, ch, cxoff, cquads, v.ppg, s));
		f->tab_w = cw; f->tab_h = ch; f->tab_xoff = cxoff; f->tab_ppg = v.ppg;
	}
	FeedRun r;
	memset(&r, 0, sizeof r);
	r.ui = v.base; r.res = res;
	r.ui_stride = v.stride; r.ui_pitch = v.pitch;
	r.w = v.w; r.h = v.h; r.xoff = v.xoff; r.quads = v.quads;
	r.n = n; r.first = first; r.flags = flags;
	r.len_term = crc32_mul(crc32_xpow(32ull * v.w * v.h), 0xFFFFFFFFu) ^ 0xFFFFFFFFu;
	r.rows_per_wave = feed_rows_per_wave(ch, n);
	r.capacity = f->capacity;
	r.raw = f->d_raw; r.tab = f->d_tab; r.state = f->d_state;
	r.header = f->d_header; r.entries = f->d_entries; r.bytes = f->d_bytes; r.maps = f->d_maps;
	*out = r;
	return SMHV_OK;
}

// The call's kernels on `s`, behind the feed's previous call (after feed_check).  v / res: the call's first frame.
static int feed_enqueue(smhv_feed *f, const FeedSrc &v, const smhv_frame_result *res, uint32_t first, uint32_t n, uint32_t flags, hipStream_t s) {
	FeedRun r;
	const int rc = feed_prepare(f, v, res, first, n, flags, s, &r);
	if (rc) return rc;
	const bool image = v.mode == SMH_RND_SRC_RGBA;
	if (v.mode == SMH_RND_SRC_UI) HIPCHK(launch_feed(r, s));
	else if (!image) HIPCHK(launch_feed_view(r, v.mode, s));
	else {
		FeedRun c = r;                                        // k_map_crc's: the rows start `lead` dwords in front of the image
		c.ui = v.base - 4ull * v.lead; c.ui_pitch = 4ull * SMH_FEED_IMAGE_ROW; c.ui_stride = 0;
		c.w = SMH_FEED_IMAGE_ROW; c.h = (uint32_t)(((uint64_t)v.w * v.h + v.lead) / SMH_FEED_IMAGE_ROW); c.xoff = 0u; c.quads = SMH_FEED_IMAGE_ROW / 4u;
		HIPCHK(launch_feed_image(c, r, s));
	}
	HIPCHK(hipEventRecord(f->ev_last, s));
	f->used = true;
	return SMHV_OK;
}

// The source of a batch call: the Map's size from the geometry alone (*v; SMHV_E_INVALID for an unknown one), and -- with
// `resolve` -- the slab it is generated from, under smhv_batch_render_layers' conditions for that source (SMHV_E_STATE).
static int feed_batch_source(const smhv_batch *b, uint32_t first, uint32_t map_source, bool resolve, FeedSrc *v) {
	const Geom &g = b->g;
	if (map_source > (uint32_t)SMHV_VIEW_CROPPED_BRQ) return fail(SMHV_E_INVALID, "batch_feed_view: unknown map source %u", map_source);
	if (resolve && !b->ui_written) return fail(SMHV_E_STATE, "batch_feed: no run of this batch has produced a ui_map (SMHV_STAGE_UI_MAP)");
	*v = feed_src_ui(g, b->d_ui + (size_t)first * g.ui_stride);
	switch ((int)map_source) {
	case SMHV_VIEW_NONE: break;
	case SMHV_VIEW_OCR_INPUT:
	case SMHV_VIEW_FIND_SCALES_INPUT: {
		const bool ocr = map_source == (uint32_t)SMHV_VIEW_OCR_INPUT;
		if (resolve && !(ocr ? b->ocr_written : b->scales_written))
			return fail(SMHV_E_STATE, "batch_feed_view: no run of this batch has produced the %s image", ocr ? "OCR input (SMHV_STAGE_OCR)" : "scales input (SMHV_STAGE_SCALES with anchors)");
		v->mode = SMH_RND_SRC_GRAY; v->ppg = 16u;
		v->base = (ocr ? b->d_ocr : b->d_scales) + (size_t)first * g.ocr_stride;
		v->pitch = g.ocr_pitch; v->stride = g.ocr_stride; v->xoff = g.q_xoff; v->w = g.qw; v->h = g.qh;
		v->quads = (v->w + v->xoff + 15u) / 16u;
		break;
	}
	case SMHV_VIEW_LSD_INPUT:
		if (resolve && !b->mask_written) return fail(SMHV_E_STATE, "batch_feed_view: no run of this batch has produced the marker mask (SMHV_STAGE_MARKERS)");
		v->mode = SMH_RND_SRC_GRAY; v->ppg = 16u;
		v->base = b->d_mask + (size_t)first * g.mask_stride;
		v->pitch = g.mask_pitch; v->stride = g.mask_stride;
		v->quads = (v->w + v->xoff + 15u) / 16u;
		break;
	default:                                                   // SMHV_VIEW_LSD_PREPROCESS, SMHV_VIEW_CROPPED_BRQ: the colour ui_map
		if (resolve && b->ui_gray) return fail(SMHV_E_STATE, "batch_feed_view: the batch's ui_map is grayscale, map source %u needs the colour one", map_source);
		if (map_source == (uint32_t)SMHV_VIEW_CROPPED_BRQ) {
			// rows from rh / 2 on, columns from m_xoff + rw / 2: whole 16-byte groups go into the base, at most 3 pixels stay a lead-in
			const uint32_t x0 = g.m_xoff + g.rw / 2u;
			v->mode = SMH_RND_SRC_CROPPED; v->w = g.rw / 2u; v->h = g.rh / 2u;
			if (resolve && (v->w == 0u || v->h == 0u)) return fail(SMHV_E_STATE, "batch_feed_view: the map has no bottom right quarter");
			v->base += (size_t)(g.rh / 2u) * g.ui_pitch + 16ull * (x0 / 4u);
			v->xoff = x0 & 3u; v->quads = (v->w + v->xoff + 3u) / 4u;
		} else v->mode = SMH_RND_SRC_PREPROCESS;
		break;
	}
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_batch_feed_view(smhv_batch *b, smhv_feed *f, uint32_t first, uint32_t n, uint32_t flags, uint32_t map_source, void *stream) {
	if (!b || !f) return fail(SMHV_E_INVALID, "batch_feed: null argument");
	CTX_OPEN(b->ctx);
	CTX_OPEN(f->ctx);
	int rc = check_device(f->ctx->device, b->ctx->device, "batch_feed", "feed", "batch");
	if (rc) return rc;
	rc = check_frames(b, first, n, "batch_feed");
	if (rc) return rc;
	FeedSrc v;
	rc = feed_batch_source(b, first, map_source, false, &v);
	if (rc) return rc;
	rc = feed_check(f, v.w, v.h, n, flags, "batch_feed");
	if (rc) return rc;
	rc = feed_batch_source(b, first, map_source, true, &v);
	if (rc) return rc;
	HIPCHK(hipSetDevice(b->ctx->device));
	if (map_source == (uint32_t)SMHV_VIEW_LSD_INPUT) {         // the mask as bytes is made when it is read (smh_runtime.cpp)
		rc = batch_materialize_mask(b, (hipStream_t)stream);
		if (rc) return rc;
	}
	rc = batch_materialize_ui(b, (hipStream_t)stream);         // ... and so is the RGBA ui slab
	if (rc) return rc;
	return feed_enqueue(f, v, b->d_results + first, first, n, flags, (hipStream_t)stream);
}

extern "C" SMHV_API int smhv_batch_feed(smhv_batch *b, smhv_feed *f, uint32_t first, uint32_t n, uint32_t flags, void *stream) {
	return smhv_batch_feed_view(b, f, first, n, flags, (uint32_t)SMHV_VIEW_NONE, stream);
}

extern "C" SMHV_API int smhv_feed_read(smhv_feed *f, smhv_feed_header *header, smhv_feed_entry *entries, uint32_t max_entries, uint8_t *bytes, uint64_t cap) {
	if (!f || !header) return fail(SMHV_E_INVALID, "feed_read: null argument");
	CTX_OPEN(f->ctx);
	HIPCHK(hipSetDevice(f->ctx->device));
	if (f->used) HIPCHK(wait_event(f->ev_last));
	HIPCHK(hipMemcpy(header, f->d_header, sizeof *header, hipMemcpyDeviceToHost));
	if (entries && header->n_entries > max_entries) return fail(SMHV_E_INVALID, "feed_read: %u entries, room for %u", header->n_entries, max_entries);
	if (bytes && header->bytes_used > cap) return fail(SMHV_E_INVALID, "feed_read: %llu bytes, room for %llu", (unsigned long long)header->bytes_used, (unsigned long long)cap);
	if (entries && header->n_entries) HIPCHK(hipMemcpy(entries, f->d_entries, sizeof(smhv_feed_entry) * header->n_entries, hipMemcpyDeviceToHost));
	if (bytes && header->bytes_used) HIPCHK(hipMemcpy(bytes, f->d_bytes, (size_t)header->bytes_used, hipMemcpyDeviceToHost));
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_feed_ptrs(smhv_feed *f, void **d_header, void **d_entries, void **d_bytes) {
	if (!f) return fail(SMHV_E_INVALID, "feed_ptrs: null feed");
	if (d_header) *d_header = f->d_header;
	if (d_entries) *d_entries = f->d_entries;
	if (d_bytes) *d_bytes = f->d_bytes;
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_debug_feed_gray_form(uint32_t form) {
	if (form != 0u && form != 4u) return fail(SMHV_E_INVALID, "feed gray form %u (0 = the rule, 4 = four lookups per message dword)", form);
	feed_set_gray_form(form);
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_debug_feed_rows(uint32_t rows) {
	if (rows > 64u) return fail(SMHV_E_INVALID, "feed rows per wave %u (0 = the rule, 1 .. 64)", rows);
	feed_set_rows(rows);
	return SMHV_OK;
}

// The current frame: frame 0 of the single-frame batch's ui slab (crop_to_map's pass) and a record made of the caller's values,
// which travels through the feed's pinned staging; on the context's stream.
extern "C" SMHV_API int smhv_feed_frame_view(smhv_ctx *c, smhv_feed *f, const smhv_line *lines, uint32_t n_lines, const double *mpx, const uint32_t minimap[4],
                                             uint32_t flags, uint32_t map_source) {
	int rc = require_open(c, "feed_frame");
	if (rc) return rc;
	CTX_OPEN(c);
	if (!f || (n_lines && !lines)) return fail(SMHV_E_INVALID, "feed_frame: null argument");
	CTX_OPEN(f->ctx);
	rc = check_device(f->ctx->device, c->device, "feed_frame", "feed", "context");
	if (rc) return rc;
	if (n_lines > SMHV_MAX_LINES) return fail(SMHV_E_INVALID, "feed_frame: %u lines (at most %u)", n_lines, (unsigned)SMHV_MAX_LINES);
	if (map_source > (uint32_t)SMHV_VIEW_CROPPED_BRQ) return fail(SMHV_E_INVALID, "feed_frame_view: unknown map source %u", map_source);
	smhv_batch *b = c->fb;
	const Geom &g = b->g;
	rc = batch_materialize_ui(b, c->s_main);                   // (the single-frame batch's pass writes RGBA: nothing is ever owed)
	if (rc) return rc;
	FeedSrc v = feed_src_ui(g, b->d_ui);
	if (map_source != (uint32_t)SMHV_VIEW_NONE) {             // smhv_get_debug_view's image of this moment, and its size
		v.mode = SMH_RND_SRC_RGBA;
		debug_view_size(g, (int)map_source, &v.w, &v.h);
		v.xoff = 0u; v.quads = 0u; v.pitch = 4ull * v.w; v.stride = 0;
	}
	rc = feed_check(f, v.w, v.h, 1, flags, "feed_frame");
	if (rc) return rc;
	HIPCHK(hipSetDevice(c->device));
	if (f->used) HIPCHK(wait_event(f->ev_last));              // (the staging record: the previous call's upload has left it; the view buffer too)
	if (v.mode == SMH_RND_SRC_RGBA) {
		// The view is drawn by smhv_get_debug_view's kernel into the feed's buffer so that it ENDS on a row of SMH_FEED_IMAGE_ROW dwords:
		// the dwords in front of it are zeroed, and the CRC reads whole aligned rows (the image itself is only 4-byte aligned).
		const uint64_t dw = (uint64_t)v.w * v.h, rows = (dw + SMH_FEED_IMAGE_ROW - 1u) / SMH_FEED_IMAGE_ROW;
		const size_t need = (size_t)rows * SMH_FEED_IMAGE_ROW * 4u;
		if (rows > SMH_FEED_MAX_ROWS) return fail(SMHV_E_INVALID, "feed_frame_view: a view of %u x %u pixels", v.w, v.h);
		if (f->view_cap < need) {
			if (f->d_view) (void)hipFree(f->d_view);
			f->d_view = nullptr; f->view_cap = 0;
			HIPCHK(hipMalloc((void **)&f->d_view, need));
			f->view_cap = need;
		}
		v.lead = (uint32_t)(rows * SMH_FEED_IMAGE_ROW - dw);
		v.base = f->d_view + 4ull * v.lead;
		if (v.lead) HIPCHK(hipMemsetAsync(f->d_view, 0, 4ull * v.lead, c->s_main));
		HIPCHK(ctx_debug_view(c, (int)map_source, f->d_view + 4ull * v.lead));
	}
	smhv_frame_result *h = f->h_rec;
	memset(h, 0, sizeof *h);
	h->map_open = 1u; h->status = SMHV_FRAME_OK;
	h->n_lines = n_lines;
	if (n_lines) memcpy(h->lines, lines, sizeof(smhv_line) * n_lines);
	if (mpx) { h->mpx = *mpx; h->has_mpx = 1u; }
	if (minimap) { memcpy(h->minimap, minimap, sizeof h->minimap); h->has_minimap = 1u; }
	HIPCHK(hipMemcpyAsync(f->d_rec, h, sizeof *h, hipMemcpyHostToDevice, c->s_main));
	return feed_enqueue(f, v, f->d_rec, 0, 1, flags, c->s_main);
}

extern "C" SMHV_API int smhv_feed_frame(smhv_ctx *c, smhv_feed *f, const smhv_line *lines, uint32_t n_lines, const double *mpx, const uint32_t minimap[4],
                                        uint32_t flags) {
	return smhv_feed_frame_view(c, f, lines, n_lines, mpx, minimap, flags, (uint32_t)SMHV_VIEW_NONE);
}

// ------------------------------------------------------------------------------------------------
// the rest of the protocol: host only
// ------------------------------------------------------------------------------------------------
static inline void web_put16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
static inline void web_put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
static inline uint32_t web_get32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// *len <- need; 0: write the message; 1: the caller only asked for the length; < 0: an error
static int web_room(const char *what, uint8_t *out, uint64_t cap, uint64_t *len, uint64_t need) {
	if (!len) return fail(SMHV_E_INVALID, "%s: null length", what);
	*len = need;
	if (!out) return 1;
	if (cap < need) return fail(SMHV_E_INVALID, "%s: %llu bytes, room for %llu", what, (unsigned long long)need, (unsigned long long)cap);
	return 0;
}

extern "C" SMHV_API int smhv_web_event_markers(const smhv_line *lines, uint32_t n, int custom, uint8_t *out, uint64_t cap, uint64_t *len) {
	if (n && !lines) return fail(SMHV_E_INVALID, "web_event_markers: null lines");
	const int rc = web_room("web_event_markers", out, cap, len, 7ull + 16ull * n);
	if (rc) return rc < 0 ? rc : SMHV_OK;
	web_put16(out, SMHV_WEB_MARKERS);
	out[2] = custom ? 1u : 0u;
	web_put32(out + 3, n);
	for (uint32_t i = 0; i < n; ++i) {
		uint32_t bits[4];
		memcpy(bits, &lines[i], sizeof bits);                 // bit for bit
		for (int k = 0; k < 4; ++k) web_put32(out + 7u + 16ull * i + 4u * k, bits[k]);
	}
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_web_event_heightmap(const uint16_t *data, uint32_t w, uint32_t h, const int32_t bounds[4], const float scale[3], uint8_t *out,
                                                 uint64_t cap, uint64_t *len) {
	if (data && (!bounds || !scale)) return fail(SMHV_E_INVALID, "web_event_heightmap: null bounds or scale");
	const uint64_t texels = data ? (uint64_t)w * h : 0ull;
	const int rc = web_room("web_event_heightmap", out, cap, len, data ? 24ull + 2ull * texels : 3ull);
	if (rc) return rc < 0 ? rc : SMHV_OK;
	web_put16(out, SMHV_WEB_HEIGHTMAP);
	if (!data) { out[2] = 0u; return SMHV_OK; }
	out[2] = 1u;
	out[3] = 0u;                                              // the pad byte: the texels start on an even offset (lib.rs:192-194)
	web_put32(out + 4, w); web_put32(out + 8, h);
	web_put32(out + 12, (uint32_t)bounds[0]); web_put32(out + 16, (uint32_t)bounds[1]);
	uint32_t z;
	memcpy(&z, &scale[2], sizeof z);
	web_put32(out + 20, z);
	for (uint64_t i = 0; i < texels; ++i) web_put16(out + 24u + 2ull * i, data[i]);
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_web_event_fit(int fit_to_minimap, uint8_t *out, uint64_t cap, uint64_t *len) {
	const int rc = web_room("web_event_fit", out, cap, len, 3ull);
	if (rc) return rc < 0 ? rc : SMHV_OK;
	web_put16(out, SMHV_WEB_FIT_TO_MINIMAP);
	out[2] = fit_to_minimap ? 1u : 0u;
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_web_interaction_parse(const uint8_t *data, uint64_t len, uint32_t *kind, float line[4], uint32_t *index) {
	if (!kind || (len && !data)) return fail(SMHV_E_INVALID, "web_interaction_parse: null argument");
	*kind = 0u;
	if (len < 2u) return SMHV_OK;
	const uint32_t id = (uint32_t)data[0] | (uint32_t)data[1] << 8;
	if (id == 1u && len == 18u) {
		if (!line) return fail(SMHV_E_INVALID, "web_interaction_parse: null line");
		for (int k = 0; k < 4; ++k) { const uint32_t bits = web_get32(data + 2 + 4 * k); memcpy(&line[k], &bits, sizeof bits); }
		*kind = 1u;
	} else if (id == 2u && len == 6u) {
		if (!index) return fail(SMHV_E_INVALID, "web_interaction_parse: null index");
		*index = web_get32(data + 2);
		*kind = 2u;
	}
	return SMHV_OK;
}
