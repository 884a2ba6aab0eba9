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
	if (paint) {
		if (!b->d_render) return fail(SMHV_E_STATE, "batch_relief: SMHV_RELIEF_PAINT and this batch has not rendered");
		rc = check_window_is_last_render(b, ropt, "batch_relief");
		if (rc) return rc;
	}
	HIPCHK(hipSetDevice(b->ctx->device));
	if (!b->d_relief) {
		hipError_t e = hipMalloc((void **)&b->d_relief, sizeof(smhv_relief_result) * (size_t)b->max_frames);
		if (e == hipSuccess) e = hipMemset(b->d_relief, 0, sizeof(smhv_relief_result) * (size_t)b->max_frames);
		if (e != hipSuccess) {
			if (b->d_relief) (void)hipFree(b->d_relief);
			b->d_relief = nullptr;
			return fail(SMHV_E_HIP, "relief slab (%u frames): %s", b->max_frames, hipGetErrorString(e));
		}
	}
	hipStream_t s = (hipStream_t)stream;
	if (paint) HIPCHK(hipStreamWaitEvent(s, b->ev_render, 0));     // behind the render (and the text passes) that drew the images
	hm_rebind(&b->relief_hm, hm);                                  // the batch's reference of the heightmap its enqueued call reads
	ReliefRun r;
	relief_run_params(hm, ropt, opt, &r);
	HIPCHK(hipMemsetAsync(b->d_relief + first, 0, sizeof(smhv_relief_result) * (size_t)n, s));
	for (uint32_t done = 0; done < n;) {                           // at most 65,535 frames per launch (the grid's third dimension)
		const uint32_t k = std::min(n - done, 65535u);
		ReliefRun part = r;
		part.aux = b->d_aux + first + done;
		part.res = b->d_results + first + done;
		part.out = b->d_relief + first + done;
		part.img = paint ? b->d_render + (size_t)(first + done) * r.img_stride : nullptr;
		part.bytes = d_bytes ? d_bytes + (size_t)done * r.plane_stride : nullptr;
		part.shades = d_shades ? d_shades + (size_t)done * r.plane_stride : nullptr;
		part.heights = d_heights ? d_heights + (size_t)done * r.plane_stride : nullptr;
		HIPCHK(launch_relief(part, k, paint, s));
		done += k;
	}
	if (paint) HIPCHK(hipEventRecord(b->ev_render, s));            // (the slab's next owner waits for the tint too)
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_batch_read_relief(smhv_batch *b, uint32_t first, uint32_t n, smhv_relief_result *out) {
	if (!b || !out || (uint64_t)first + n > b->max_frames) return fail(SMHV_E_INVALID, "batch_read_relief: bad arguments");
	if (!b->d_relief) return fail(SMHV_E_STATE, "batch_read_relief: this batch has computed no relief");
	return batch_read_rows(b, b->d_relief, sizeof(smhv_relief_result), first, n, out);
}

extern "C" SMHV_API int smhv_batch_relief_ptr(smhv_batch *b, void **d_relief) {
	if (!b || !d_relief) return fail(SMHV_E_INVALID, "batch_relief_ptr: null argument");
	if (!b->d_relief) return fail(SMHV_E_STATE, "batch_relief_ptr: this batch has computed no relief");
	*d_relief = b->d_relief;
	return SMHV_OK;
}

// The per-call path: the caller's image up, the kernels, the image, the planes and the summary down, through the context's pinned
// block (smhv_firing_solutions' buffers, grown on demand; fire_mu from sizing them to the last copy).
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
	r.per_call = 1u;
	r.has_mm = minimap ? 1u : 0u;
	if (minimap) memcpy(r.mm, minimap, sizeof r.mm);
	// [the summary, 256 bytes][the flag bytes][the shades][the heights][the image], each part on a 256-byte boundary
	const auto pad = [](size_t v) { return (v + 255u) & ~(size_t)255u; };
	const size_t px = (size_t)r.plane_stride;
	const size_t bytes_off = 256u, bytes_len = bytes ? px : 0u, shades_off = bytes_off + pad(bytes_len), shades_len = shades ? px : 0u;
	const size_t heights_off = shades_off + pad(shades_len), heights_len = heights ? px * sizeof(float) : 0u;
	const size_t img_off = heights_off + pad(heights_len), img_len = rgba_inout ? (size_t)r.img_stride : 0u, total = img_off + img_len;
	std::lock_guard<std::mutex> lk(c->fire_mu);
	rc = ctx_stage_reserve(c, total);
	if (rc) return rc;
	r.out = (smhv_relief_result *)c->d_fire;
	r.bytes = bytes ? c->d_fire + bytes_off : nullptr;
	r.shades = shades ? c->d_fire + shades_off : nullptr;
	r.heights = heights ? (float *)(c->d_fire + heights_off) : nullptr;
	r.img = rgba_inout ? c->d_fire + img_off : nullptr;
	HIPCHK(hipMemsetAsync(c->d_fire, 0, sizeof(smhv_relief_result), c->s_main));
	if (rgba_inout) {
		memcpy(c->h_fire + img_off, rgba_inout, img_len);
		HIPCHK(hipMemcpyAsync(c->d_fire + img_off, c->h_fire + img_off, img_len, hipMemcpyHostToDevice, c->s_main));
	}
	HIPCHK(launch_relief(r, 1, rgba_inout != nullptr, c->s_main));
	HIPCHK(hipMemcpyAsync(c->h_fire, c->d_fire, total, hipMemcpyDeviceToHost, c->s_main));
	HIPCHK(wait_stream(c->s_main));
	if (rgba_inout) memcpy(rgba_inout, c->h_fire + img_off, img_len);
	if (bytes) memcpy(bytes, c->h_fire + bytes_off, bytes_len);
	if (shades) memcpy(shades, c->h_fire + shades_off, shades_len);
	if (heights) memcpy(heights, c->h_fire + heights_off, heights_len);
	if (result) memcpy(result, c->h_fire, sizeof *result);
	return SMHV_OK;
}
