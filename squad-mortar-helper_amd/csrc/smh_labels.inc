// smh_labels.inc -- the marker labels of the map view: public entry points (smh_vision_hip.h, "map view: labels"; device code in
// smh_labels.hip).  Included at the end of smh_runtime.cpp, after smh_render.inc.
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
	const size_t frames = (size_t)b->max_frames, extra_bytes = sizeof(smhv_label_line) * SMHV_LABEL_MAX_EXTRA;
	int rc = first_use_slabs(b, "label slab (%u frames)", {{(void **)&b->d_labels, sizeof(smhv_label_result) * frames, 0},
	                                                       {(void **)&b->d_label_cull, sizeof(LabelCull) * SMH_LBL_SLOTS * frames, 0},
	                                                       {(void **)&b->d_label_extra, extra_bytes, SLAB_NO_FILL},
	                                                       {(void **)&b->h_label_extra, extra_bytes, SLAB_PINNED_HOST}});
	if (rc) return rc;
	if (lo->n_extra) {
		if (!b->ev_label_extra) HIPCHK(hipEventCreateWithFlags(&b->ev_label_extra, hipEventDisableTiming));
		else HIPCHK(wait_event(b->ev_label_extra));
		memcpy(b->h_label_extra, lo->extra, sizeof(smhv_label_line) * (size_t)lo->n_extra);
		HIPCHK(hipMemcpyAsync(b->d_label_extra, b->h_label_extra, sizeof(smhv_label_line) * (size_t)lo->n_extra, hipMemcpyHostToDevice, s));
		HIPCHK(hipEventRecord(b->ev_label_extra, s));
	}
	memset(r, 0, sizeof *r);
	const smhv_firing_options fo = firing_opts_of_render(ropt);
	firing_run_params(hm, &fo, &r->fr);
	r->extra = b->d_label_extra;
	r->n_extra = lo->n_extra;
	r->detected = lo->flags & SMHV_LABEL_DETECTED;
	r->scale = lo->scale ? lo->scale : 2u;
	r->out_w = ropt->out_w; r->out_h = ropt->out_h;
	r->img_stride = (uint64_t)ropt->out_w * ropt->out_h * 4u;
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_batch_render_labels(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *ropt,
                                                 const smhv_label_options *lopt, void *stream) {
	if (!b) return fail(SMHV_E_INVALID, "batch_render_labels: null batch");
	CTX_OPEN(b->ctx);
	int rc = check_render_options(ropt, hm, "batch_render_labels");
	if (rc) return rc;
	rc = check_label_options(lopt, "batch_render_labels");
	if (rc) return rc;
	rc = check_frames(b, first, n, "batch_render_labels");
	if (rc) return rc;
	rc = check_hm_device(hm, b->ctx->device, "batch_render_labels", "batch");
	if (rc) return rc;
	if (!b->d_render) return fail(SMHV_E_STATE, "batch_render_labels: this batch has not rendered");
	rc = check_window_is_last_render(b, ropt, "batch_render_labels");
	if (rc) return rc;
	HIPCHK(hipSetDevice(b->ctx->device));
	hipStream_t s = (hipStream_t)stream;
	// behind the render that drew the images, whatever stream it took -- and behind the previous label call's kernels, which read
	// the device copy of the extras that labels_prepare overwrites on `s` (ev_render is recorded again at the end of this call)
	HIPCHK(hipStreamWaitEvent(s, b->ev_render, 0));
	LabelRun r;
	rc = labels_prepare(b, hm, ropt, lopt, s, &r);
	if (rc) return rc;
	hm_rebind(&b->label_hm, hm);                               // the batch's reference of the heightmap its enqueued labels read
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
	return batch_read_slab(b, b ? b->d_labels : nullptr, sizeof(smhv_label_result), first, n, out, "batch_read_labels", "this batch has drawn no labels");
}

extern "C" SMHV_API int smhv_batch_labels_ptr(smhv_batch *b, void **d_labels) {
	return batch_slab_ptr(b, b ? b->d_labels : nullptr, d_labels, "batch_labels_ptr", "this batch has drawn no labels");
}

// the per-call path: render_map_per_call (smh_render.inc) with the labels over the image
extern "C" SMHV_API int smhv_render_map_labeled(smhv_ctx *c, const smhv_heightmap *hm, const smhv_render_options *opt, const smhv_render_layers *layers,
                                                const smhv_line *lines, uint32_t n_lines, const smhv_label_options *lopt, uint8_t *rgba,
                                                smhv_label_result *labels) {
	return render_map_per_call(c, hm, opt, layers, lines, n_lines, lopt, nullptr, rgba, labels, nullptr, PER_CALL_TEXT, "render_map_labeled");
}
