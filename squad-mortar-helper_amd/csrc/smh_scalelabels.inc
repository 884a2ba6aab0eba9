// smh_scalelabels.inc -- scale labels: public entry points (smh_vision_hip.h, "scale labels"; device code in smh_scalelabels.hip).
// Included at the end of smh_runtime.cpp.

// The family's slabs, by the first call: the records, the crops, and S0 -- a plane of the family's own, filled by the quadrant pass
// with start row 0 from the frames' pixels (the batch's scales plane keeps the rows of its own run's start row, and its readers
// their image).
static int scale_labels_slabs(smhv_batch *b) {
	const size_t frames = b->max_frames;
	return first_use_slabs(b, "scale label slabs (%u frames)", {{(void **)&b->d_sl, sizeof(smhv_scale_label_frame) * frames, 0},
	                                                            {(void **)&b->d_sl_crops, (size_t)SMHV_LABEL_FRAME_CROP_BYTES * frames, 255},
	                                                            {(void **)&b->d_sl_s0, (size_t)b->g.ocr_stride * frames, SLAB_NO_FILL}});
}

static int check_scale_labels_geom(const Geom &g, const char *what) {
	if (g.ocr_pitch > SMH_SL_MAX_DIM || g.qh > SMH_SL_MAX_DIM)
		return fail(SMHV_E_GEOMETRY, "%s: a quadrant of %u x %u (a padded row of at most %u bytes and at most %u rows)", what, g.qw, g.qh, SMH_SL_MAX_DIM, SMH_SL_MAX_DIM);
	return SMHV_OK;
}

// S0, then the kernel, over frames [0, n) of b on s; frames: the pixels the ocr plane was made from
static int scale_labels_enqueue(smhv_batch *b, const uint8_t *frames, uint32_t n, hipStream_t s) {
	const Geom &g = b->g;
	Buffers bf{};                                             // (the quadrant pass reads frames, aux and writes scales: nothing else of a run's block)
	bf.frames = frames; bf.aux = b->d_aux; bf.anchors = b->d_anchors;
	bf.ocr = b->d_ocr; bf.scales = b->d_sl_s0;
	HIPCHK(launch_brq_pass(g, bf, n, BRQ_SCALES, 0, 0, s));
	ScaleLabelsRun r{};
	r.aux = b->d_aux; r.ocr = b->d_ocr; r.s0 = b->d_sl_s0;
	r.out = b->d_sl; r.crops = b->d_sl_crops;
	r.stride = g.ocr_stride; r.pitch = (uint32_t)g.ocr_pitch; r.q_xoff = g.q_xoff; r.qw = g.qw; r.qh = g.qh;
	r.gap = scale_labels_gap(g.qw);
	HIPCHK(launch_scale_labels(r, n, s));
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_batch_scale_labels(smhv_batch *b, const void *d_frames, uint32_t n, void *stream) {
	if (!b) return fail(SMHV_E_INVALID, "batch_scale_labels: null batch");
	CTX_OPEN(b->ctx);
	if (!d_frames) return fail(SMHV_E_INVALID, "batch_scale_labels: null d_frames");
	if ((uintptr_t)d_frames & 3u) return fail(SMHV_E_INVALID, "batch_scale_labels: d_frames is not aligned to a pixel (4 bytes)");
	int rc = check_frames(b, 0, n, "batch_scale_labels");
	if (rc) return rc;
	rc = check_scale_labels_geom(b->g, "batch_scale_labels");
	if (rc) return rc;
	if (!(b->run_stages & SMHV_STAGE_OCR)) return fail(SMHV_E_STATE, "batch_scale_labels: the batch's last run had no SMHV_STAGE_OCR");
	if (n > b->run_n) return fail(SMHV_E_STATE, "batch_scale_labels: %u frames, the batch's last run covered %u", n, b->run_n);
	HIPCHK(hipSetDevice(b->ctx->device));
	rc = scale_labels_slabs(b);
	if (rc) return rc;
	rc = scale_labels_enqueue(b, (const uint8_t *)d_frames, n, (hipStream_t)stream);
	if (rc == SMHV_OK) b->sl_n = n;                            // (smhv_batch_label_text: the labels of these frames are on their way)
	return rc;
}

extern "C" SMHV_API int smhv_batch_read_scale_labels(smhv_batch *b, uint32_t first, uint32_t n, smhv_scale_label_frame *out, uint8_t *crops) {
	const int rc = batch_read_slab(b, b ? b->d_sl : nullptr, sizeof(smhv_scale_label_frame), first, n, out, "batch_read_scale_labels", "this batch has computed no scale labels");
	if (rc || !crops) return rc;
	return batch_read_rows(b, b->d_sl_crops, SMHV_LABEL_FRAME_CROP_BYTES, first, n, crops);
}

extern "C" SMHV_API int smhv_batch_scale_labels_ptr(smhv_batch *b, void **d_labels, void **d_crops) {
	if (!b) return fail(SMHV_E_INVALID, "batch_scale_labels_ptr: null batch");
	if (!b->d_sl) return fail(SMHV_E_STATE, "batch_scale_labels_ptr: this batch has computed no scale labels");
	if (d_labels) *d_labels = b->d_sl;
	if (d_crops) *d_crops = b->d_sl_crops;
	return SMHV_OK;
}

// The per-call path: on the scales branch's stream, behind smhv_ocr_preprocess' pass; the record and the cells come down through the
// context's pinned block (fire_mu from sizing it to the last copy).
extern "C" SMHV_API int smhv_scale_labels(smhv_ctx *c, smhv_scale_label_frame *out, uint8_t *crops) {
	int rc = require_open(c, "scale_labels");
	if (rc) return rc;
	CTX_OPEN(c);
	if (!out) return fail(SMHV_E_INVALID, "scale_labels: null output");
	if (!c->ocr_valid) return fail(SMHV_E_STATE, "scale_labels called before ocr_preprocess on this frame");
	smhv_batch *b = c->fb;
	rc = check_scale_labels_geom(b->g, "scale_labels");
	if (rc) return rc;
	HIPCHK(hipSetDevice(c->device));
	rc = scale_labels_slabs(b);
	if (rc) return rc;
	hipStream_t s = c->s_scales;
	// [the record][the cells], each part on a 256-byte boundary
	StageLayout lay;
	lay.take(sizeof(smhv_scale_label_frame));
	const StagePart cells = lay.part(crops, (size_t)SMHV_LABEL_FRAME_CROP_BYTES);
	std::lock_guard<std::mutex> lk(c->fire_mu);
	rc = ctx_stage_reserve(c, lay.total());
	if (rc) return rc;
	rc = scale_labels_enqueue(b, c->frame_ptr, 1, s);
	if (rc) return rc;
	HIPCHK(hipMemcpyAsync(c->h_fire, b->d_sl, sizeof(smhv_scale_label_frame), hipMemcpyDeviceToHost, s));
	if (crops) HIPCHK(hipMemcpyAsync(c->h_fire + cells.off, b->d_sl_crops, cells.len, hipMemcpyDeviceToHost, s));
	HIPCHK(wait_stream(s));
	b->sl_n = 1; c->labels_valid = true;                       // (smhv_label_text)
	memcpy(out, c->h_fire, sizeof *out);
	if (crops) memcpy(crops, c->h_fire + cells.off, (size_t)std::min(out->n, (uint32_t)SMHV_MAX_SCALE_LABELS) * SMHV_LABEL_CROP_BYTES);
	return SMHV_OK;
}

// src/vision/mod.rs:161-186 on numbers the host has read, and the ladder of mpx_ratio.rs:91-125 on the proposals' own widths
extern "C" SMHV_API int smhv_scale_labels_anchors(const smhv_scale_label *labels, uint32_t n, const uint32_t *meters, smhv_anchors *out, double *mpx, int *has) {
	if ((n && (!labels || !meters)) || n > 65536u) return fail(SMHV_E_INVALID, "scale_labels_anchors: bad arguments");
	smhv_anchors an;
	double ratio = 0.0;
	uint32_t bad = 0;
	if (!label_anchors(labels, n, meters, &an, &ratio, &bad))  // (smh_glyph_rule.h: the text the device runs on the meters it reads)
		return fail(SMHV_E_INVALID, "scale_labels_anchors: label %u has no bar (%u .. %u)", bad, labels[bad].bar_left, labels[bad].bar_right);
	if (out) *out = an;
	if (has) *has = an.n ? 1 : 0;
	if (mpx) *mpx = ratio;
	return SMHV_OK;
}
