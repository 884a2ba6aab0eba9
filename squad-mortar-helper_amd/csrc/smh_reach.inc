// smh_reach.inc -- the reach map: public entry points (smh_vision_hip.h, "reach map"; device code in smh_reach.hip, the pixel rule
// in smh_firing.h).  Included at the end of smh_runtime.cpp.

extern "C" SMHV_API int smhv_reach_thresholds(double out[7]) {
	static const double T[7] = SMH_REACH_THRESHOLDS;
	if (!out) return fail(SMHV_E_INVALID, "reach_thresholds: null argument");
	memcpy(out, T, sizeof T);
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_reach_defaults(smhv_reach_options *opt) {
	static const uint8_t band[8][4] = {{40, 90, 255, 72}, {0, 170, 255, 72}, {0, 220, 200, 72}, {0, 230, 110, 72},
	                                   {120, 235, 0, 72}, {220, 230, 0, 72}, {255, 180, 0, 72}, {255, 120, 40, 72}};
	static const uint8_t oor[4] = {200, 30, 30, 96}, ring[4] = {255, 255, 255, 160};
	if (!opt) return fail(SMHV_E_INVALID, "reach_defaults: null options");
	memset(opt, 0, sizeof *opt);
	opt->size = sizeof *opt;
	opt->flags = SMHV_REACH_PAINT;
	opt->origin_mode = SMHV_REACH_ORIGIN_POINT;
	memcpy(opt->out_of_range, oor, 4);
	memcpy(opt->band, band, sizeof band);
	memcpy(opt->ring, ring, 4);
	return SMHV_OK;
}

// what a call can get wrong in its reach options without the device being asked
static int check_reach_options(const smhv_reach_options *o, const char *what) {
	if (!o) return fail(SMHV_E_INVALID, "%s: null reach options", what);
	if (o->size != sizeof(smhv_reach_options)) return fail(SMHV_E_INVALID, "%s: smhv_reach_options.size %u != %zu", what, o->size, sizeof(smhv_reach_options));
	if (o->flags & ~(SMHV_REACH_PAINT | SMHV_REACH_CLASSES)) return fail(SMHV_E_INVALID, "%s: unknown reach flags 0x%x", what, o->flags);
	if (o->origin_mode > SMHV_REACH_ORIGIN_LINE_P1) return fail(SMHV_E_INVALID, "%s: origin mode %u", what, o->origin_mode);
	if (o->origin_mode != SMHV_REACH_ORIGIN_POINT && o->line >= (uint32_t)SMHV_MAX_LINES)
		return fail(SMHV_E_INVALID, "%s: line %u (a record holds %u)", what, o->line, (unsigned)SMHV_MAX_LINES);
	if (!std::isfinite(o->ring_m) || o->ring_m < 0.0) return fail(SMHV_E_INVALID, "%s: ring_m %g (finite, >= 0)", what, o->ring_m);
	return SMHV_OK;
}

// the launch arguments but for the frames' own pointers
static void reach_run_params(const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_reach_options *o, ReachRun *r) {
	memset(r, 0, sizeof *r);
	const smhv_firing_options fo = firing_opts_of_render(ropt);
	firing_run_params(hm, &fo, &r->fr);
	r->out_w = ropt->out_w; r->out_h = ropt->out_h;
	r->img_stride = (uint64_t)ropt->out_w * ropt->out_h * 4u;
	r->cls_stride = (uint64_t)ropt->out_w * ropt->out_h;
	r->ring_m = o->ring_m;
	r->origin[0] = o->origin[0]; r->origin[1] = o->origin[1];
	r->origin_mode = o->origin_mode; r->line = o->line;
	memcpy(&r->pal[0], o->out_of_range, 4);
	memcpy(&r->pal[1], o->band, 32);
	memcpy(&r->pal[9], o->ring, 4);
}

extern "C" SMHV_API int smhv_batch_reach(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *ropt,
                                         const smhv_reach_options *opt, void *d_classes, void *stream) {
	if (!b) return fail(SMHV_E_INVALID, "batch_reach: null batch");
	CTX_OPEN(b->ctx);
	int rc = check_render_options(ropt, hm, "batch_reach");
	if (rc) return rc;
	rc = check_reach_options(opt, "batch_reach");
	if (rc) return rc;
	rc = check_frames(b, first, n, "batch_reach");
	if (rc) return rc;
	rc = check_hm_device(hm, b->ctx->device, "batch_reach", "batch");
	if (rc) return rc;
	const bool paint = (opt->flags & SMHV_REACH_PAINT) != 0u, classes = (opt->flags & SMHV_REACH_CLASSES) != 0u;
	if (classes && !d_classes) return fail(SMHV_E_INVALID, "batch_reach: SMHV_REACH_CLASSES and a null d_classes");
	ReachRun r;
	reach_run_params(hm, ropt, opt, &r);
	hipStream_t s = (hipStream_t)stream;
	return window_pass_batch(b, first, n, hm, ropt, r, paint, "SMHV_REACH_PAINT", &b->d_reach, "reach slab (%u frames)", &b->reach_hm, s, "batch_reach",
	                         [&](ReachRun &part, uint32_t done, uint32_t k) -> int {
		part.cls = classes ? (uint8_t *)d_classes + (size_t)done * r.cls_stride : nullptr;
		HIPCHK(launch_reach(part, k, paint, classes, s));
		return SMHV_OK;
	});
}

extern "C" SMHV_API int smhv_batch_read_reach(smhv_batch *b, uint32_t first, uint32_t n, smhv_reach_result *out) {
	return batch_read_slab(b, b ? b->d_reach : nullptr, sizeof(smhv_reach_result), first, n, out, "batch_read_reach", "this batch has computed no reach map");
}

extern "C" SMHV_API int smhv_batch_reach_ptr(smhv_batch *b, void **d_reach) {
	return batch_slab_ptr(b, b ? b->d_reach : nullptr, d_reach, "batch_reach_ptr", "this batch has computed no reach map");
}

// The per-call path (window_pass_per_call): the caller's image up, the kernel, the image, the classes and the summary down.
extern "C" SMHV_API int smhv_reach_map(smhv_ctx *c, const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_reach_options *opt, const double *mpx,
                                       const uint32_t minimap[4], uint8_t *rgba_inout, uint8_t *classes, smhv_reach_result *result) {
	if (!c) return fail(SMHV_E_INVALID, "reach_map: null context");
	CTX_OPEN(c);
	if (!rgba_inout && !classes) return fail(SMHV_E_INVALID, "reach_map: neither an image nor a class buffer");
	int rc = check_render_options(ropt, hm, "reach_map");
	if (rc) return rc;
	rc = check_reach_options(opt, "reach_map");
	if (rc) return rc;
	if (opt->origin_mode != SMHV_REACH_ORIGIN_POINT) return fail(SMHV_E_INVALID, "reach_map: origin mode %u (the per-call path takes SMHV_REACH_ORIGIN_POINT only)", opt->origin_mode);
	rc = check_hm_device(hm, c->device, "reach_map", "context");
	if (rc) return rc;
	HIPCHK(hipSetDevice(c->device));
	ReachRun r;
	reach_run_params(hm, ropt, opt, &r);
	r.has_mpx = mpx ? 1u : 0u; r.mpx = mpx ? *mpx : 0.0;
	// [the summary, 256 bytes][the classes][the image], each part on a 256-byte boundary
	StageLayout lay;
	lay.take(256u);
	const StagePart cls = lay.part(classes, (size_t)r.cls_stride), img = lay.part(rgba_inout, (size_t)r.img_stride);
	return window_pass_per_call(c, r, minimap, lay.total(), img, {cls, {result, 0, sizeof *result}}, [&](ReachRun &run, uint8_t *block, hipStream_t s) -> int {
		run.cls = classes ? block + cls.off : nullptr;
		HIPCHK(launch_reach(run, 1, rgba_inout != nullptr, classes != nullptr, s));
		return SMHV_OK;
	});
}
