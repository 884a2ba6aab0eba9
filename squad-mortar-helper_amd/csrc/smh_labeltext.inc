// smh_labeltext.inc -- scale labels: text: public entry points (smh_vision_hip.h, "scale labels: text"; the rule in smh_glyph_rule.h,
// device code in smh_labeltext.hip).  Included at the end of smh_runtime.cpp.

// a device copy of a glyph atlas (smhv_glyph_atlas_create)
struct smhv_glyph_atlas {
	smhv_ctx *ctx = nullptr;
	GlyphAtlas *d = nullptr;
};

static int glyph_templates_check(const smhv_glyph_template *t, uint32_t n, const char *what) {
	if (!t) return fail(SMHV_E_INVALID, "%s: null templates", what);
	if (n == 0u || n > SMHV_ATLAS_MAX_TEMPLATES) return fail(SMHV_E_INVALID, "%s: %u templates (1 .. %u)", what, n, SMHV_ATLAS_MAX_TEMPLATES);
	for (uint32_t i = 0; i < n; ++i)
		if (const char *why = glyph_template_fault(&t[i])) return fail(SMHV_E_INVALID, "%s: template %u: %s", what, i, why);
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_glyph_templates_check(const smhv_glyph_template *templates, uint32_t n) {
	return glyph_templates_check(templates, n, "glyph_templates_check");
}

extern "C" SMHV_API int smhv_glyph_templates_from_label(const uint8_t *crop, const smhv_scale_label *label, const char *text, smhv_glyph_template *out, uint32_t *n) {
	if (!crop || !label || !text || !out || !n) return fail(SMHV_E_INVALID, "glyph_templates_from_label: null argument");
	*n = 0;
	if (label->right <= label->left || label->bottom <= label->top || label->right - label->left > SMHV_LABEL_CROP_W || label->bottom - label->top > SMHV_LABEL_CROP_H)
		return fail(SMHV_E_INVALID, "glyph_templates_from_label: a box of %u .. %u x %u .. %u (at most %u x %u)", label->left, label->right, label->top, label->bottom, SMHV_LABEL_CROP_W, SMHV_LABEL_CROP_H);
	const size_t len = strlen(text);
	uint64_t lo[32], hi[32], olo, ohi;
	label_row_masks(crop, label->right - label->left, label->bottom - label->top, lo, hi, &olo, &ohi);
	smhv_glyph_template tmp[SMHV_LABEL_MAX_GLYPHS];
	uint32_t k = 0, l = 0, r = 0;
	for (uint32_t from = 0; glyph_next_run(olo, ohi, from, &l, &r); from = r + 1u, ++k) {
		if (k >= SMHV_LABEL_MAX_GLYPHS || k >= len) continue;  // (counted: the message names the true count)
		uint32_t g[32], gw, gh;
		label_glyph(lo, hi, l, r, g, &gw, &gh);
		if (gw > 32u) return fail(SMHV_E_INVALID, "glyph_templates_from_label: glyph %u is %u columns wide (at most 32)", k, gw);
		memset(&tmp[k], 0, sizeof tmp[k]);
		tmp[k].code = (uint8_t)text[k]; tmp[k].w = (uint8_t)gw; tmp[k].h = (uint8_t)gh;
		memcpy(tmp[k].rows, g, sizeof g);
		if (const char *why = glyph_template_fault(&tmp[k])) return fail(SMHV_E_INVALID, "glyph_templates_from_label: glyph %u ('%c'): %s", k, text[k], why);
	}
	if (k != len || k > SMHV_LABEL_MAX_GLYPHS)
		return fail(SMHV_E_INVALID, "glyph_templates_from_label: %u glyphs for a text of %zu characters (at most %u)", k, len, SMHV_LABEL_MAX_GLYPHS);
	memcpy(out, tmp, sizeof(smhv_glyph_template) * k);
	*n = k;
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_glyph_atlas_create(smhv_ctx *c, const smhv_glyph_template *templates, uint32_t n, const smhv_glyph_atlas_options *options, smhv_glyph_atlas **out) {
	if (!c || !out) return fail(SMHV_E_INVALID, "glyph_atlas_create: null argument");
	*out = nullptr;
	CTX_OPEN(c);
	int rc = glyph_templates_check(templates, n, "glyph_atlas_create");
	if (rc) return rc;
	const uint32_t num = options ? options->accept_num : 1u, den = options ? options->accept_den : 3u;
	if (den == 0u) return fail(SMHV_E_INVALID, "glyph_atlas_create: accept_den is 0");
	HIPCHK(hipSetDevice(c->device));
	smhv_glyph_atlas *a = new (std::nothrow) smhv_glyph_atlas();
	GlyphAtlas *h = new (std::nothrow) GlyphAtlas;
	if (!a || !h) { delete a; delete h; return fail(SMHV_E_INVALID, "out of host memory"); }
	glyph_atlas_fill(h, templates, n, num, den);
	hipError_t e = hipMalloc((void **)&a->d, sizeof(GlyphAtlas));
	if (e == hipSuccess) e = hipMemcpy(a->d, h, sizeof(GlyphAtlas), hipMemcpyHostToDevice);
	delete h;
	if (e != hipSuccess) {
		if (a->d) (void)hipFree(a->d);
		delete a;
		return fail(SMHV_E_HIP, "glyph_atlas_create: %s", hipGetErrorString(e));
	}
	c->refs.fetch_add(1, std::memory_order_relaxed);
	a->ctx = c;
	*out = a;
	return SMHV_OK;
}

extern "C" SMHV_API void smhv_glyph_atlas_destroy(smhv_glyph_atlas *a) {
	if (!a) return;
	(void)hipSetDevice(a->ctx->device);
	(void)hipDeviceSynchronize();                              // (work that reads the atlas may still be enqueued)
	if (a->d) (void)hipFree(a->d);
	ctx_release(a->ctx);
	delete a;
}

// the family's slabs, by the first call
static int label_text_slabs(smhv_batch *b) {
	const size_t frames = b->max_frames;
	return first_use_slabs(b, "label text slabs (%u frames)", {{(void **)&b->d_lt, sizeof(smhv_label_text_frame) * frames, 0},
	                                                           {(void **)&b->d_lt_anchors, sizeof(smhv_anchors) * frames, 0}});
}

static int label_text_enqueue(smhv_batch *b, const smhv_glyph_atlas *a, uint32_t n, hipStream_t s) {
	LabelTextRun r{};
	r.labels = b->d_sl; r.crops = b->d_sl_crops; r.atlas = a->d;
	r.out = b->d_lt; r.anchors = b->d_lt_anchors;
	HIPCHK(launch_label_text(r, n, s));
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_batch_label_text(smhv_batch *b, const smhv_glyph_atlas *atlas, uint32_t n, void *stream) {
	if (!b) return fail(SMHV_E_INVALID, "batch_label_text: null batch");
	CTX_OPEN(b->ctx);
	if (!atlas) return fail(SMHV_E_INVALID, "batch_label_text: null atlas");
	int rc = check_frames(b, 0, n, "batch_label_text");
	if (rc) return rc;
	rc = check_device(atlas->ctx->device, b->ctx->device, "batch_label_text", "glyph atlas", "batch");
	if (rc) return rc;
	if (!b->d_sl || n > b->sl_n) return fail(SMHV_E_STATE, "batch_label_text: %u frames, the batch's last smhv_batch_scale_labels covered %u", n, b->d_sl ? b->sl_n : 0u);
	HIPCHK(hipSetDevice(b->ctx->device));
	rc = label_text_slabs(b);
	if (rc) return rc;
	rc = label_text_enqueue(b, atlas, n, (hipStream_t)stream);
	if (rc == SMHV_OK) b->lt_n = n;
	return rc;
}

extern "C" SMHV_API int smhv_batch_read_label_text(smhv_batch *b, uint32_t first, uint32_t n, smhv_label_text_frame *out) {
	return batch_read_slab(b, b ? b->d_lt : nullptr, sizeof(smhv_label_text_frame), first, n, out, "batch_read_label_text", "this batch has read no label text");
}

extern "C" SMHV_API int smhv_batch_label_text_ptr(smhv_batch *b, void **d_text, void **d_anchors) {
	if (!b) return fail(SMHV_E_INVALID, "batch_label_text_ptr: null batch");
	if (!b->d_lt) return fail(SMHV_E_STATE, "batch_label_text_ptr: this batch has read no label text");
	if (d_text) *d_text = b->d_lt;
	if (d_anchors) *d_anchors = b->d_lt_anchors;
	return SMHV_OK;
}

// The per-call path: on the scales branch's stream, behind smhv_scale_labels' kernels; the record comes down through the context's
// pinned block.
extern "C" SMHV_API int smhv_label_text(smhv_ctx *c, const smhv_glyph_atlas *atlas, smhv_label_text_frame *out) {
	int rc = require_open(c, "label_text");
	if (rc) return rc;
	CTX_OPEN(c);
	if (!atlas || !out) return fail(SMHV_E_INVALID, "label_text: null argument");
	rc = check_device(atlas->ctx->device, c->device, "label_text", "glyph atlas", "context");
	if (rc) return rc;
	smhv_batch *b = c->fb;
	if (!c->ocr_valid || !c->labels_valid || !b->d_sl) return fail(SMHV_E_STATE, "label_text called before scale_labels on this frame");
	HIPCHK(hipSetDevice(c->device));
	rc = label_text_slabs(b);
	if (rc) return rc;
	hipStream_t s = c->s_scales;
	std::lock_guard<std::mutex> lk(c->fire_mu);
	rc = ctx_stage_reserve(c, sizeof(smhv_label_text_frame));
	if (rc) return rc;
	rc = label_text_enqueue(b, atlas, 1, s);
	if (rc) return rc;
	b->lt_n = 1;
	HIPCHK(hipMemcpyAsync(c->h_fire, b->d_lt, sizeof(smhv_label_text_frame), hipMemcpyDeviceToHost, s));
	HIPCHK(wait_stream(s));
	memcpy(out, c->h_fire, sizeof *out);
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_batch_run_label_anchors(smhv_batch *b, const void *d_frames, uint32_t n, uint32_t stages, int grayscale, uint32_t max_gap, void *stream) {
	if (!b) return fail(SMHV_E_INVALID, "batch_run_label_anchors: null batch");
	CTX_OPEN(b->ctx);
	if (n == 0u || n > b->max_frames) return fail(SMHV_E_INVALID, "batch_run_label_anchors: %u frames of a batch of %u", n, b->max_frames);
	if (!b->d_lt_anchors || n > b->lt_n) return fail(SMHV_E_STATE, "batch_run_label_anchors: %u frames, the batch's last smhv_batch_label_text covered %u", n, b->d_lt_anchors ? b->lt_n : 0u);
	return batch_run_impl(b, d_frames, n, stages, grayscale, max_gap, nullptr, (hipStream_t)stream, (hipStream_t)stream, nullptr, b->d_lt_anchors);
}
