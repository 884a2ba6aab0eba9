// smh_relief.inc -- terrain relief: public entry points (smh_vision_hip.h, "terrain relief"; device code in smh_relief.hip).
// Included at the end of smh_runtime.cpp.

extern "C" SMHV_API int smhv_relief_defaults(smhv_relief_options *opt) {
	static const uint8_t contour[4] = {60, 40, 20, 110}, major[4] = {60, 40, 20, 200};
	if (!opt) return fail(SMHV_E_INVALID, "relief_defaults: null options");
	memset(opt, 0, sizeof *opt);
	opt->size = sizeof *opt;
	opt->flags = SMHV_RELIEF_PAINT;
	opt->major_every = 5u;
	opt->interval_m = 10.0;
	opt->exaggeration = 1.0;
	opt->light[0] = -0.5; opt->light[1] = -0.5; opt->light[2] = 0x1.6a09e667f3bcdp-1;   // north-west, 45 degrees up
	memcpy(opt->contour, contour, 4);
	memcpy(opt->major, major, 4);
	opt->shade_weight = 96u;
	return SMHV_OK;
}

// what a call can get wrong in its relief options without the device being asked
static int check_relief_options(const smhv_relief_options *o, const char *what) {
	if (!o) return fail(SMHV_E_INVALID, "%s: null relief options", what);
	if (o->size != sizeof(smhv_relief_options)) return fail(SMHV_E_INVALID, "%s: smhv_relief_options.size %u != %zu", what, o->size, sizeof(smhv_relief_options));
	if (o->flags & ~(SMHV_RELIEF_PAINT | SMHV_RELIEF_BYTES | SMHV_RELIEF_SHADES | SMHV_RELIEF_HEIGHTS | SMHV_RELIEF_NEAREST))
		return fail(SMHV_E_INVALID, "%s: unknown relief flags 0x%x", what, o->flags);
	if (!std::isfinite(o->interval_m) || o->interval_m < 0.0) return fail(SMHV_E_INVALID, "%s: interval_m %g (finite, >= 0)", what, o->interval_m);
	if (!std::isfinite(o->base_m)) return fail(SMHV_E_INVALID, "%s: base_m %g is not finite", what, o->base_m);
	if (!std::isfinite(o->exaggeration)) return fail(SMHV_E_INVALID, "%s: exaggeration %g is not finite", what, o->exaggeration);
	for (int i = 0; i < 3; ++i)
		if (!std::isfinite(o->light[i])) return fail(SMHV_E_INVALID, "%s: light[%d] is not finite", what, i);
	if (o->shade_weight > 255u) return fail(SMHV_E_INVALID, "%s: shade_weight %u (at most 255)", what, o->shade_weight);
	return SMHV_OK;
}

// the launch arguments but for the frames' own pointers
static void relief_run_params(const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_relief_options *o, ReliefRun *r) {
	memset(r, 0, sizeof *r);
	const smhv_firing_options fo = firing_opts_of_render(ropt);
	firing_run_params(hm, &fo, &r->fr);
	r->out_w = ropt->out_w; r->out_h = ropt->out_h;
	r->img_stride = (uint64_t)ropt->out_w * ropt->out_h * 4u;
	r->plane_stride = (uint64_t)ropt->out_w * ropt->out_h;
	r->interval_m = o->interval_m; r->base_m = o->base_m; r->exaggeration = o->exaggeration;
	r->light[0] = o->light[0]; r->light[1] = o->light[1]; r->light[2] = o->light[2];
	r->nearest = (o->flags & SMHV_RELIEF_NEAREST) ? 1u : 0u;
	r->major_every = o->major_every;
	r->shade_weight = o->shade_weight;
	memcpy(&r->pal[0], o->contour, 4);
	memcpy(&r->pal[1], o->major, 4);
}

extern "C" SMHV_API int smhv_batch_relief(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *ropt,
                                          const smhv_relief_options *opt, const smhv_relief_planes *planes, void *stream) {
	if (!b) return fail(SMHV_E_INVALID, "batch_relief: null batch");
	CTX_OPEN(b->ctx);
	if (!hm) return fail(SMHV_E_INVALID, "batch_relief: null heightmap (relief without terrain is nothing)");
	int rc = check_render_options(ropt, hm, "batch_relief");
	if (rc) return rc;
	rc = check_relief_options(opt, "batch_relief");
	if (rc) return rc;
	rc = check_frames(b, first, n, "batch_relief");
	if (rc) return rc;
	rc = check_hm_device(hm, b->ctx->device, "batch_relief", "batch");
	if (rc) return rc;
	const bool paint = (opt->flags & SMHV_RELIEF_PAINT) != 0u;
	uint8_t *d_bytes = nullptr, *d_shades = nullptr;
	float *d_heights = nullptr;
	if (opt->flags & SMHV_RELIEF_BYTES) {
		if (!planes || !planes->bytes) return fail(SMHV_E_INVALID, "batch_relief: SMHV_RELIEF_BYTES and a null bytes plane");
		d_bytes = (uint8_t *)planes->bytes;
	}
	if (opt->flags & SMHV_RELIEF_SHADES) {
		if (!planes || !planes->shades) return fail(SMHV_E_INVALID, "batch_relief: SMHV_RELIEF_SHADES and a null shades plane");
		d_shades = (uint8_t *)planes->shades;
	}
	if (opt->flags & SMHV_RELIEF_HEIGHTS) {
		if (!planes || !planes->heights) return fail(SMHV_E_INVALID, "batch_relief: SMHV_RELIEF_HEIGHTS and a null heights plane");
		d_heights = (float *)planes->heights;
	}
	ReliefRun r;
	relief_run_params(hm, ropt, opt, &r);
	hipStream_t s = (hipStream_t)stream;
	return window_pass_batch(b, first, n, hm, ropt, r, paint, "SMHV_RELIEF_PAINT", &b->d_relief, "relief slab (%u frames)", &b->relief_hm, s, "batch_relief",
	                         [&](ReliefRun &part, uint32_t done, uint32_t k) -> int {
		part.bytes = d_bytes ? d_bytes + (size_t)done * r.plane_stride : nullptr;
		part.shades = d_shades ? d_shades + (size_t)done * r.plane_stride : nullptr;
		part.heights = d_heights ? d_heights + (size_t)done * r.plane_stride : nullptr;
		HIPCHK(launch_relief(part, k, paint, s));
		return SMHV_OK;
	});
}

extern "C" SMHV_API int smhv_batch_read_relief(smhv_batch *b, uint32_t first, uint32_t n, smhv_relief_result *out) {
	return batch_read_slab(b, b ? b->d_relief : nullptr, sizeof(smhv_relief_result), first, n, out, "batch_read_relief", "this batch has computed no relief");
}

extern "C" SMHV_API int smhv_batch_relief_ptr(smhv_batch *b, void **d_relief) {
	return batch_slab_ptr(b, b ? b->d_relief : nullptr, d_relief, "batch_relief_ptr", "this batch has computed no relief");
}

// The per-call path (window_pass_per_call): the caller's image up, the kernels, the image, the planes and the summary down.
extern "C" SMHV_API int smhv_relief_map(smhv_ctx *c, const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_relief_options *opt,
                                        const uint32_t minimap[4], uint8_t *rgba_inout, uint8_t *bytes, uint8_t *shades, float *heights,
                                        smhv_relief_result *result) {
	if (!c) return fail(SMHV_E_INVALID, "relief_map: null context");
	CTX_OPEN(c);
	if (!hm) return fail(SMHV_E_INVALID, "relief_map: null heightmap (relief without terrain is nothing)");
	if (!rgba_inout && !bytes && !shades && !heights && !result) return fail(SMHV_E_INVALID, "relief_map: no output");
	int rc = check_render_options(ropt, hm, "relief_map");
	if (rc) return rc;
	rc = check_relief_options(opt, "relief_map");
	if (rc) return rc;
	rc = check_hm_device(hm, c->device, "relief_map", "context");
	if (rc) return rc;
	HIPCHK(hipSetDevice(c->device));
	ReliefRun r;
	relief_run_params(hm, ropt, opt, &r);
	// [the summary, 256 bytes][the flag bytes][the shades][the heights][the image], each part on a 256-byte boundary
	StageLayout lay;
	lay.take(256u);
	const size_t px = (size_t)r.plane_stride;
	const StagePart pb = lay.part(bytes, px), ps = lay.part(shades, px), ph = lay.part(heights, px * sizeof(float)), img = lay.part(rgba_inout, (size_t)r.img_stride);
	return window_pass_per_call(c, r, minimap, lay.total(), img, {pb, ps, ph, {result, 0, sizeof *result}}, [&](ReliefRun &run, uint8_t *block, hipStream_t s) -> int {
		run.bytes = bytes ? block + pb.off : nullptr;
		run.shades = shades ? block + ps.off : nullptr;
		run.heights = heights ? (float *)(block + ph.off) : nullptr;
		HIPCHK(launch_relief(run, 1, rgba_inout != nullptr, s));
		return SMHV_OK;
	});
}
