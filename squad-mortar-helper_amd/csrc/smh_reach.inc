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
	if (paint) {
		if (!b->d_render) return fail(SMHV_E_STATE, "batch_reach: SMHV_REACH_PAINT and this batch has not rendered");
		rc = check_window_is_last_render(b, ropt, "batch_reach");
		if (rc) return rc;
	}
	HIPCHK(hipSetDevice(b->ctx->device));
	if (!b->d_reach) {
		hipError_t e = hipMalloc((void **)&b->d_reach, sizeof(smhv_reach_result) * (size_t)b->max_frames);
		if (e == hipSuccess) e = hipMemset(b->d_reach, 0, sizeof(smhv_reach_result) * (size_t)b->max_frames);
		if (e != hipSuccess) {
			if (b->d_reach) (void)hipFree(b->d_reach);
			b->d_reach = nullptr;
			return fail(SMHV_E_HIP, "reach slab (%u frames): %s", b->max_frames, hipGetErrorString(e));
		}
	}
	hipStream_t s = (hipStream_t)stream;
	if (paint) HIPCHK(hipStreamWaitEvent(s, b->ev_render, 0));     // behind the render (and the text passes) that drew the images
	hm_rebind(&b->reach_hm, hm);                                   // the batch's reference of the heightmap its enqueued call reads
	ReachRun r;
	reach_run_params(hm, ropt, opt, &r);
	HIPCHK(hipMemsetAsync(b->d_reach + first, 0, sizeof(smhv_reach_result) * (size_t)n, s));
	for (uint32_t done = 0; done < n;) {                           // at most 65,535 frames per launch (the grid's third dimension)
		const uint32_t k = std::min(n - done, 65535u);
		ReachRun part = r;
		part.aux = b->d_aux + first + done;
		part.res = b->d_results + first + done;
		part.out = b->d_reach + first + done;
		part.img = paint ? b->d_render + (size_t)(first + done) * r.img_stride : nullptr;
		part.cls = classes ? (uint8_t *)d_classes + (size_t)done * r.cls_stride : nullptr;
		HIPCHK(launch_reach(part, k, paint, classes, s));
		done += k;
	}
	if (paint) HIPCHK(hipEventRecord(b->ev_render, s));            // (the slab's next owner waits for the tint too)
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_batch_read_reach(smhv_batch *b, uint32_t first, uint32_t n, smhv_reach_result *out) {
	if (!b || !out || (uint64_t)first + n > b->max_frames) return fail(SMHV_E_INVALID, "batch_read_reach: bad arguments");
	if (!b->d_reach) return fail(SMHV_E_STATE, "batch_read_reach: this batch has computed no reach map");
	return batch_read_rows(b, b->d_reach, sizeof(smhv_reach_result), first, n, out);
}

extern "C" SMHV_API int smhv_batch_reach_ptr(smhv_batch *b, void **d_reach) {
	if (!b || !d_reach) return fail(SMHV_E_INVALID, "batch_reach_ptr: null argument");
	if (!b->d_reach) return fail(SMHV_E_STATE, "batch_reach_ptr: this batch has computed no reach map");
	*d_reach = b->d_reach;
	return SMHV_OK;
}

// The per-call path: the caller's image up, the kernel, the image, the classes and the summary down, through the context's pinned
// block (smhv_firing_solutions' buffers, grown on demand; fire_mu from sizing them to the last copy).
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
	r.per_call = 1u;
	r.has_mpx = mpx ? 1u : 0u; r.mpx = mpx ? *mpx : 0.0;
	r.has_mm = minimap ? 1u : 0u;
	if (minimap) memcpy(r.mm, minimap, sizeof r.mm);
	// [the summary, 256 bytes][the classes][the image], each part on a 256-byte boundary
	const size_t cls_off = 256u, cls_bytes = classes ? (size_t)r.cls_stride : 0u, img_off = cls_off + ((cls_bytes + 255u) & ~(size_t)255u);
	const size_t img_bytes = rgba_inout ? (size_t)r.img_stride : 0u, bytes = img_off + img_bytes;
	std::lock_guard<std::mutex> lk(c->fire_mu);
	rc = ctx_stage_reserve(c, bytes);
	if (rc) return rc;
	r.out = (smhv_reach_result *)c->d_fire;
	r.cls = classes ? c->d_fire + cls_off : nullptr;
	r.img = rgba_inout ? c->d_fire + img_off : nullptr;
	HIPCHK(hipMemsetAsync(c->d_fire, 0, sizeof(smhv_reach_result), c->s_main));
	if (rgba_inout) {
		memcpy(c->h_fire + img_off, rgba_inout, img_bytes);
		HIPCHK(hipMemcpyAsync(c->d_fire + img_off, c->h_fire + img_off, img_bytes, hipMemcpyHostToDevice, c->s_main));
	}
	HIPCHK(launch_reach(r, 1, rgba_inout != nullptr, classes != nullptr, c->s_main));
	HIPCHK(hipMemcpyAsync(c->h_fire, c->d_fire, bytes, hipMemcpyDeviceToHost, c->s_main));
	HIPCHK(wait_stream(c->s_main));
	if (rgba_inout) memcpy(rgba_inout, c->h_fire + img_off, img_bytes);
	if (classes) memcpy(classes, c->h_fire + cls_off, cls_bytes);
	if (result) memcpy(result, c->h_fire, sizeof *result);
	return SMHV_OK;
}
