// smh_labels.inc -- the marker labels of the map view: public entry points (smh_vision_hip.h, "map view: labels"; device code in
// smh_labels.hip).  Included at the end of smh_runtime.cpp.
#include "smh_font5x7.h"

extern "C" SMHV_API int smhv_label_font(uint8_t ch, uint8_t rows[7]) {
	static const uint8_t font[SMH_FONT_GLYPHS][SMH_FONT_ROWS] = SMH_FONT5X7_TABLE;
	if (!rows) return fail(SMHV_E_INVALID, "label_font: null rows");
	const int g = smh_font_index(ch);
	if (g < 0) return fail(SMHV_E_INVALID, "label_font: the font has no glyph for byte 0x%02x", ch);
	memcpy(rows, font[g], SMH_FONT_ROWS);
	return SMHV_OK;
}

// what a call can get wrong in its label options without the device being asked
static int check_label_options(const smhv_label_options *lo, const char *what) {
	if (!lo) return fail(SMHV_E_INVALID, "%s: null label options", what);
	if (lo->size != sizeof(smhv_label_options)) return fail(SMHV_E_INVALID, "%s: smhv_label_options.size %u != %zu", what, lo->size, sizeof(smhv_label_options));
	if (lo->flags & ~SMHV_LABEL_DETECTED) return fail(SMHV_E_INVALID, "%s: unknown label flags 0x%x", what, lo->flags);
	if (lo->scale > 4u) return fail(SMHV_E_INVALID, "%s: label scale %u (1 .. 4, 0 = 2)", what, lo->scale);
	if (lo->n_extra > SMHV_LABEL_MAX_EXTRA) return fail(SMHV_E_INVALID, "%s: %u extra lines (at most %u)", what, lo->n_extra, SMHV_LABEL_MAX_EXTRA);
	if (lo->n_extra && !lo->extra) return fail(SMHV_E_INVALID, "%s: %u extra lines and a null pointer", what, lo->n_extra);
	for (uint32_t i = 0; i < lo->n_extra; ++i)
		if (lo->extra[i].rgba[3] != 255u) return fail(SMHV_E_INVALID, "%s: extra line %u has alpha %u (255 only)", what, i, lo->extra[i].rgba[3]);
	return SMHV_OK;
}

// The batch's label buffers (first call), the extras through pinned staging onto `s` (waits, host, for the previous call's copy to
// have read the staging), and the launch arguments but for the frames' own pointers.
static int labels_prepare(smhv_batch *b, const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_label_options *lo, hipStream_t s, LabelRun *r) {
	if (!b->d_labels) {
		const size_t frames = (size_t)b->max_frames;
		hipError_t e = hipMalloc((void **)&b->d_labels, sizeof(smhv_label_result) * frames);
		if (e == hipSuccess) e = hipMalloc((void **)&b->d_label_cull, sizeof(LabelCull) * SMH_LBL_SLOTS * frames);
		if (e == hipSuccess) e = hipMalloc((void **)&b->d_label_extra, sizeof(smhv_label_line) * SMHV_LABEL_MAX_EXTRA);
		if (e == hipSuccess) e = hipHostMalloc((void **)&b->h_label_extra, sizeof(smhv_label_line) * SMHV_LABEL_MAX_EXTRA, hipHostMallocDefault);
		if (e == hipSuccess) e = hipMemset(b->d_labels, 0, sizeof(smhv_label_result) * frames);
		if (e == hipSuccess) e = hipMemset(b->d_label_cull, 0, sizeof(LabelCull) * SMH_LBL_SLOTS * frames);
		if (e != hipSuccess) {
			if (b->d_labels) (void)hipFree(b->d_labels);
			if (b->d_label_cull) (void)hipFree(b->d_label_cull);
			if (b->d_label_extra) (void)hipFree(b->d_label_extra);
			if (b->h_label_extra) (void)hipHostFree(b->h_label_extra);
			b->d_labels = nullptr; b->d_label_cull = nullptr; b->d_label_extra = nullptr; b->h_label_extra = nullptr;
			return fail(SMHV_E_HIP, "label slab (%u frames): %s", b->max_frames, hipGetErrorString(e));
		}
	}
	if (lo->n_extra) {
		if (!b->ev_label_extra) HIPCHK(hipEventCreateWithFlags(&b->ev_label_extra, hipEventDisableTiming));
		else HIPCHK(wait_event(b->ev_label_extra));
		memcpy(b->h_label_extra, lo->extra, sizeof(smhv_label_line) * (size_t)lo->n_extra);
		HIPCHK(hipMemcpyAsync(b->d_label_extra, b->h_label_extra, sizeof(smhv_label_line) * (size_t)lo->n_extra, hipMemcpyHostToDevice, s));
		HIPCHK(hipEventRecord(b->ev_label_extra, s));
	}
	memset(r, 0, sizeof *r);
	smhv_firing_options fo{};
	fo.size = sizeof fo;
	fo.flags = (ropt->flags & SMHV_RENDER_BOUNDS_OFFSET) ? SMHV_FIRING_BOUNDS_OFFSET : 0u;
	fo.viewport_scale[0] = ropt->viewport_scale[0]; fo.viewport_scale[1] = ropt->viewport_scale[1];
	fo.viewport_top_left[0] = ropt->viewport_top_left[0]; fo.viewport_top_left[1] = ropt->viewport_top_left[1];
	firing_run_params(hm, &fo, &r->fr);
	r->extra = b->d_label_extra;
	r->n_extra = lo->n_extra;
	r->detected = lo->flags & SMHV_LABEL_DETECTED;
	r->scale = lo->scale ? lo->scale : 2u;
	r->out_w = ropt->out_w; r->out_h = ropt->out_h;
	r->img_stride = (uint64_t)ropt->out_w * ropt->out_h * 4u;
	return SMHV_OK;
}

// the batch's reference of the heightmap its enqueued labels read (as render_bind)
static void labels_bind(smhv_batch *b, const smhv_heightmap *hm) {
	smhv_heightmap *h = const_cast<smhv_heightmap *>(hm);
	if (b->label_hm == h) return;
	hm_retain(h);
	smhv_heightmap *old = b->label_hm;
	b->label_hm = h;
	hm_release(old);
}

extern "C" SMHV_API int smhv_batch_render_labels(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *ropt,
                                                 const smhv_label_options *lopt, void *stream) {
	if (!b) return fail(SMHV_E_INVALID, "batch_render_labels: null batch");
	CTX_OPEN(b->ctx);
	int rc = check_render_options(ropt, hm, "batch_render_labels");
	if (rc) return rc;
	rc = check_label_options(lopt, "batch_render_labels");
	if (rc) return rc;
	if (n == 0u || (uint64_t)first + n > b->max_frames) return fail(SMHV_E_INVALID, "batch_render_labels: frames [%u, %u + %u) of a batch of %u", first, first, n, b->max_frames);
	if (hm && hm->ctx->device != b->ctx->device) return fail(SMHV_E_INVALID, "batch_render_labels: the heightmap lives on device %d, the batch on %d", hm->ctx->device, b->ctx->device);
	if (!b->d_render) return fail(SMHV_E_STATE, "batch_render_labels: this batch has not rendered");
	if (ropt->out_w != b->render_w || ropt->out_h != b->render_h)
		return fail(SMHV_E_STATE, "batch_render_labels: a window of %u x %u, the batch's most recent render is %u x %u", ropt->out_w, ropt->out_h, b->render_w, b->render_h);
	HIPCHK(hipSetDevice(b->ctx->device));
	hipStream_t s = (hipStream_t)stream;
	// behind the render that drew the images, whatever stream it took -- and behind the previous label call's kernels, which read
	// the device copy of the extras that labels_prepare overwrites on `s` (ev_render is recorded again at the end of this call)
	HIPCHK(hipStreamWaitEvent(s, b->ev_render, 0));
	LabelRun r;
	rc = labels_prepare(b, hm, ropt, lopt, s, &r);
	if (rc) return rc;
	labels_bind(b, hm);
	r.aux = b->d_aux + first;
	r.res = b->d_results + first;
	r.out = b->d_labels + first;
	r.cull = b->d_label_cull + (size_t)first * SMH_LBL_SLOTS;
	r.img = b->d_render + (size_t)first * r.img_stride;
	HIPCHK(launch_labels(r, n, s));
	HIPCHK(hipEventRecord(b->ev_render, s));                   // (the slab's next owner waits for the labels too)
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_batch_read_labels(smhv_batch *b, uint32_t first, uint32_t n, smhv_label_result *out) {
	if (!b || !out || (uint64_t)first + n > b->max_frames) return fail(SMHV_E_INVALID, "batch_read_labels: bad arguments");
	if (!b->d_labels) return fail(SMHV_E_STATE, "batch_read_labels: this batch has drawn no labels");
	HIPCHK(hipSetDevice(b->ctx->device));
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpy(out, b->d_labels + first, sizeof(smhv_label_result) * n, hipMemcpyDeviceToHost));
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_batch_labels_ptr(smhv_batch *b, void **d_labels) {
	if (!b || !d_labels) return fail(SMHV_E_INVALID, "batch_labels_ptr: null argument");
	if (!b->d_labels) return fail(SMHV_E_STATE, "batch_labels_ptr: this batch has drawn no labels");
	*d_labels = b->d_labels;
	return SMHV_OK;
}

// The per-call path.  The image is smhv_render_map's / smhv_render_map_layers's: their enqueueing is restated here (those entry
// points copy the image out themselves, and this one copies it once, after the labels), launch for launch.  smhv_render_map_debug
// (smh_debugtext.inc) is the same call with the debug pass behind the labels: dopt != NULL, checked by its caller, and lopt may
// then be NULL (no labels).
static int debug_prepare(smhv_batch *b, const smhv_render_options *ropt, const smhv_debug_options *dopt, bool draw, hipStream_t s, DebugRun *r);
static int render_map_text(smhv_ctx *c, const smhv_heightmap *hm, const smhv_render_options *opt, const smhv_render_layers *layers, const smhv_line *lines,
                           uint32_t n_lines, const smhv_label_options *lopt, const smhv_debug_options *dopt, uint8_t *rgba, smhv_label_result *labels,
                           smhv_probe *probes, const char *what) {
	int rc = require_open(c, what);
	if (rc) return rc;
	CTX_OPEN(c);
	if (!rgba || (n_lines && !lines)) return fail(SMHV_E_INVALID, "%s: null argument", what);
	if (n_lines > SMHV_RENDER_MAX_LINES) return fail(SMHV_E_INVALID, "%s: %u lines (at most %u)", what, n_lines, SMHV_RENDER_MAX_LINES);
	rc = check_render_options(opt, hm, what);
	if (rc) return rc;
	if (layers) {
		rc = check_render_layers(layers, what);
		if (rc) return rc;
	}
	if (lopt || !dopt) {
		rc = check_label_options(lopt, what);
		if (rc) return rc;
	}
	if (lopt && (lopt->flags & SMHV_LABEL_DETECTED) && n_lines > SMHV_MAX_LINES)
		return fail(SMHV_E_INVALID, "%s: %u detected lines to label (at most %u)", what, n_lines, (unsigned)SMHV_MAX_LINES);
	if (hm && hm->ctx->device != c->device) return fail(SMHV_E_INVALID, "%s: the heightmap lives on device %d, the context on %d", what, hm->ctx->device, c->device);
	HIPCHK(hipSetDevice(c->device));
	smhv_batch *b = c->fb;
	const Geom &g = b->g;
	const bool use_hm = (opt->flags & SMHV_RENDER_HEIGHTMAP) != 0u;
	std::lock_guard<std::mutex> lk(c->fire_mu);
	RenderRun r;
	rc = render_prepare(b, 0, 1, b->d_results + 3, use_hm ? hm : nullptr, opt, &r);
	if (rc) return rc;
	RenderLayersRun y{};
	uint8_t *d_view = nullptr;
	if (layers) {
		y.flags = layers->flags;
		y.src_mode = SMH_RND_SRC_UI; y.src_w = g.rw; y.src_h = g.rh;
		if (layers->map_source != (uint32_t)SMHV_VIEW_NONE) {
			const int which = (int)layers->map_source;
			const bool brq = which == SMHV_VIEW_OCR_INPUT || which == SMHV_VIEW_FIND_SCALES_INPUT || which == SMHV_VIEW_CROPPED_BRQ;
			y.src_w = brq ? g.qw : g.rw; y.src_h = brq ? g.qh : g.rh;
			HIPCHK(hipMalloc((void **)&d_view, (size_t)y.src_w * y.src_h * 4u));
			Buffers bf = make_buffers(b, c->frame_ptr, 0);
			hipError_t e = launch_debug_view(g, bf, 0, which, c->isolated ? 1 : 0, d_view, c->s_main);
			if (e != hipSuccess) { (void)hipFree(d_view); return fail(SMHV_E_HIP, "%s: debug view: %s", what, hipGetErrorString(e)); }
			y.src_mode = SMH_RND_SRC_RGBA; y.src = d_view; y.src_pitch = (uint64_t)y.src_w * 4u;
		}
	}
	const auto run = [&]() -> int {
		const size_t line_bytes = sizeof(smhv_line) * (size_t)SMHV_RENDER_MAX_LINES;
		if (c->fire_cap < line_bytes) {
			if (c->d_fire) (void)hipFree(c->d_fire);
			if (c->h_fire) (void)hipHostFree(c->h_fire);
			c->d_fire = c->h_fire = nullptr; c->fire_cap = 0;
			HIPCHK(hipMalloc((void **)&c->d_fire, line_bytes));
			HIPCHK(hipHostMalloc((void **)&c->h_fire, line_bytes));
			c->fire_cap = line_bytes;
		}
		const bool label_lines = lopt && n_lines && (lopt->flags & SMHV_LABEL_DETECTED);
		if (n_lines && ((opt->flags & SMHV_RENDER_MARKERS) || label_lines)) {
			memcpy(c->h_fire, lines, sizeof(smhv_line) * (size_t)n_lines);
			HIPCHK(hipMemcpyAsync(c->d_fire, c->h_fire, sizeof(smhv_line) * (size_t)n_lines, hipMemcpyHostToDevice, c->s_main));
		}
		if (n_lines && (opt->flags & SMHV_RENDER_MARKERS)) { r.lines = (const smhv_line *)c->d_fire; r.n_lines = n_lines; }
		else r.flags &= ~SMHV_RENDER_MARKERS;                    // (no explicit lines: none are drawn, whatever the spare record holds)
		if (layers) {
			int rc2 = render_upload_prims(b, layers, &y, c->s_main);
			if (rc2) return rc2;
			HIPCHK(launch_render_map_layers(g, r, y, 1, c->s_main));
		} else
			HIPCHK(launch_render_map(g, r, 1, c->s_main));
		if (lopt) {
			LabelRun lr;
			int rc2 = labels_prepare(b, hm, opt, lopt, c->s_main, &lr);
			if (rc2) return rc2;
			lr.aux = b->d_aux;
			lr.res = b->d_results + 3;
			lr.per_call = 1u;
			lr.lines = label_lines ? (const smhv_line *)c->d_fire : nullptr;
			lr.n_lines = label_lines ? n_lines : 0u;
			lr.has_mpx = lopt->mpx ? 1u : 0u;
			lr.mpx = lopt->mpx ? *lopt->mpx : 0.0;
			lr.out = b->d_labels;
			lr.cull = b->d_label_cull;
			lr.img = b->d_render;
			HIPCHK(launch_labels(lr, 1, c->s_main));
		}
		if (dopt) {
			DebugRun dr;
			int rc2 = debug_prepare(b, opt, dopt, true, c->s_main, &dr);
			if (rc2) return rc2;
			rc2 = batch_materialize_ui(b, c->s_main);              // (the single-frame batch's pass writes RGBA: nothing is ever owed)
			if (rc2) return rc2;
			dr.ui = b->d_ui;
			dr.aux = b->d_aux;
			dr.res = b->d_results + 3;
			dr.probes = b->d_probes;
			dr.items = b->d_dbg_items;
			dr.pool = b->d_dbg_pool;
			dr.img = b->d_render;
			HIPCHK(launch_debug_text(g, dr, 1, c->s_main));
			HIPCHK(hipEventRecord(b->ev_dbg, c->s_main));
			b->probed = true;
		}
		HIPCHK(hipEventRecord(b->ev_render, c->s_main));
		std::lock_guard<std::mutex> lk2(c->mu);                  // (staging slot 2: the batch read-back's)
		int rc3 = copy_image_d2h(c, 2, rgba, b->d_render, (size_t)r.out_stride / opt->out_h, 0, (size_t)opt->out_w * 4, opt->out_h, c->s_main);
		if (rc3) return rc3;
		if (labels && lopt) HIPCHK(hipMemcpy(labels, b->d_labels, sizeof(smhv_label_result), hipMemcpyDeviceToHost));   // (the stream has run dry)
		if (probes && dopt) HIPCHK(hipMemcpy(probes, b->d_probes, sizeof(smhv_probe) * SMHV_MAX_PROBES, hipMemcpyDeviceToHost));
		return SMHV_OK;
	};
	rc = run();
	if (d_view) {
		if (rc) (void)hipStreamSynchronize(c->s_main);           // (whatever was enqueued has left the view before it goes)
		(void)hipFree(d_view);
	}
	return rc;
}

extern "C" SMHV_API int smhv_render_map_labeled(smhv_ctx *c, const smhv_heightmap *hm, const smhv_render_options *opt, const smhv_render_layers *layers,
                                                const smhv_line *lines, uint32_t n_lines, const smhv_label_options *lopt, uint8_t *rgba,
                                                smhv_label_result *labels) {
	return render_map_text(c, hm, opt, layers, lines, n_lines, lopt, nullptr, rgba, labels, nullptr, "render_map_labeled");
}
