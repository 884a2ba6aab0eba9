// smh_clear.inc -- terrain clearance: public entry points (smh_vision_hip.h, "terrain clearance"; device code in smh_clear.hip, the
// steps of the rule in smh_firing.h).  Included at the end of smh_runtime.cpp.

extern "C" SMHV_API int smhv_clearance_defaults(smhv_clearance_options *opt) {
	static const uint8_t blocked[4] = {230, 40, 40, 110}, los[4] = {0, 0, 0, 70};
	if (!opt) return fail(SMHV_E_INVALID, "clearance_defaults: null options");
	memset(opt, 0, sizeof *opt);
	opt->size = sizeof *opt;
	opt->flags = SMHV_CLEAR_PAINT;
	opt->samples = 64u;
	opt->origin_mode = SMHV_REACH_ORIGIN_POINT;
	memcpy(opt->blocked, blocked, 4);
	memcpy(opt->los, los, 4);
	return SMHV_OK;
}

// what a call can get wrong in its clearance options without the device being asked (`map`: the origin fields apply)
static int check_clearance_options(const smhv_clearance_options *o, bool map, const char *what) {
	if (!o) return fail(SMHV_E_INVALID, "%s: null clearance options", what);
	if (o->size != sizeof(smhv_clearance_options))
		return fail(SMHV_E_INVALID, "%s: smhv_clearance_options.size %u != %zu", what, o->size, sizeof(smhv_clearance_options));
	if (o->flags & ~(SMHV_CLEAR_PAINT | SMHV_CLEAR_BYTES)) return fail(SMHV_E_INVALID, "%s: unknown clearance flags 0x%x", what, o->flags);
	if (o->samples == 0u || o->samples > SMHV_CLEAR_MAX_SAMPLES)
		return fail(SMHV_E_INVALID, "%s: %u samples (1 .. %u)", what, o->samples, (unsigned)SMHV_CLEAR_MAX_SAMPLES);
	if (!std::isfinite(o->margin_m) || o->margin_m < 0.0) return fail(SMHV_E_INVALID, "%s: margin_m %g (finite, >= 0)", what, o->margin_m);
	if (map) {
		if (o->origin_mode > SMHV_REACH_ORIGIN_LINE_P1) return fail(SMHV_E_INVALID, "%s: origin mode %u", what, o->origin_mode);
		if (o->origin_mode != SMHV_REACH_ORIGIN_POINT && o->line >= (uint32_t)SMHV_MAX_LINES)
			return fail(SMHV_E_INVALID, "%s: line %u (a record holds %u)", what, o->line, (unsigned)SMHV_MAX_LINES);
	}
	return SMHV_OK;
}

// ---- the lines
extern "C" SMHV_API int smhv_batch_clearance(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_firing_options *fopt,
                                             const smhv_clearance_options *opt, void *d_profiles, void *stream) {
	if (!b) return fail(SMHV_E_INVALID, "batch_clearance: null batch");
	CTX_OPEN(b->ctx);
	int rc = check_firing_options(fopt);
	if (rc) return rc;
	rc = check_clearance_options(opt, false, "batch_clearance");
	if (rc) return rc;
	rc = check_frames(b, first, n, "batch_clearance");
	if (rc) return rc;
	rc = check_hm_device(hm, b->ctx->device, "batch_clearance", "batch");
	if (rc) return rc;
	HIPCHK(hipSetDevice(b->ctx->device));
	rc = first_use_slabs(b, "clearance slab (%u frames)", {{(void **)&b->d_clear, sizeof(smhv_clearance_result) * (size_t)b->max_frames, 0}});
	if (rc) return rc;
	hipStream_t s = (hipStream_t)stream;
	hm_rebind(&b->clear_hm, hm);                                   // the batch's reference of the heightmap its enqueued call reads
	const smhv_firing_options fo = firing_opts(fopt);
	ClearLinesRun r;
	memset(&r, 0, sizeof r);
	firing_run_params(hm, &fo, &r.fr);
	r.margin_m = opt->margin_m;
	r.samples = opt->samples;
	return for_each_launch(n, [&](uint32_t done, uint32_t k) -> int {
		ClearLinesRun part = r;
		part.res = b->d_results + first + done;
		part.out = b->d_clear + first + done;
		part.profiles = d_profiles ? (float *)d_profiles + (size_t)done * SMHV_MAX_LINES * SMH_CLEAR_PROFILE : nullptr;
		HIPCHK(launch_clear_lines(part, k, s));
		return SMHV_OK;
	});
}

extern "C" SMHV_API int smhv_batch_read_clearance(smhv_batch *b, uint32_t first, uint32_t n, smhv_clearance_result *out) {
	return batch_read_slab(b, b ? b->d_clear : nullptr, sizeof(smhv_clearance_result), first, n, out, "batch_read_clearance", "this batch has computed no clearance");
}

extern "C" SMHV_API int smhv_batch_clearance_ptr(smhv_batch *b, void **d_clearance) {
	return batch_slab_ptr(b, b ? b->d_clear : nullptr, d_clearance, "batch_clearance_ptr", "this batch has computed no clearance");
}

// The per-call path: the lines up, the kernel, the records and the profiles down, through the context's pinned block.
extern "C" SMHV_API int smhv_clearance_lines(smhv_ctx *c, const smhv_line *lines, uint32_t n, const uint32_t minimap[4], const smhv_heightmap *hm,
                                             const smhv_firing_options *fopt, const smhv_clearance_options *opt, smhv_clearance *out, float *profiles) {
	if (!c || (n && (!lines || !out))) return fail(SMHV_E_INVALID, "clearance_lines: null argument");
	CTX_OPEN(c);
	int rc = check_firing_options(fopt);
	if (rc) return rc;
	rc = check_clearance_options(opt, false, "clearance_lines");
	if (rc) return rc;
	if (n == 0) return SMHV_OK;
	rc = check_hm_device(hm, c->device, "clearance_lines", "context");
	if (rc) return rc;
	HIPCHK(hipSetDevice(c->device));
	const smhv_firing_options fo = firing_opts(fopt);
	ClearLinesRun r;
	memset(&r, 0, sizeof r);
	firing_run_params(hm, &fo, &r.fr);
	r.margin_m = opt->margin_m;
	r.samples = opt->samples;
	r.per_call = 1u; r.n_lines = n;
	r.has_mm = minimap ? 1u : 0u;
	if (minimap) memcpy(r.mm, minimap, sizeof r.mm);
	// [the lines][the records][the profiles], each part on a 256-byte boundary
	StageLayout lay;
	const size_t in_bytes = sizeof(smhv_line) * (size_t)n;
	lay.take(in_bytes);
	const StagePart rec = lay.part(out, sizeof(smhv_clearance) * (size_t)n), prof = lay.part(profiles, sizeof(float) * SMH_CLEAR_PROFILE * (size_t)n);
	std::lock_guard<std::mutex> lk(c->fire_mu);
	rc = ctx_stage_reserve(c, lay.total());
	if (rc) return rc;
	r.lines = (const smhv_line *)c->d_fire;
	r.out_lines = (smhv_clearance *)(c->d_fire + rec.off);
	r.profiles = profiles ? (float *)(c->d_fire + prof.off) : nullptr;
	memcpy(c->h_fire, lines, in_bytes);
	HIPCHK(hipMemcpyAsync(c->d_fire, c->h_fire, in_bytes, hipMemcpyHostToDevice, c->s_main));
	HIPCHK(launch_clear_lines(r, 1, c->s_main));
	HIPCHK(hipMemcpyAsync(c->h_fire + rec.off, c->d_fire + rec.off, lay.total() - rec.off, hipMemcpyDeviceToHost, c->s_main));   // the records and the profiles: not the lines
	HIPCHK(wait_stream(c->s_main));
	memcpy(out, c->h_fire + rec.off, rec.len);
	if (profiles) memcpy(profiles, c->h_fire + prof.off, prof.len);
	return SMHV_OK;
}

// ---- the map
// the launch arguments but for the frames' own pointers
static void clear_map_params(const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_clearance_options *o, ClearMapRun *r) {
	memset(r, 0, sizeof *r);
	const smhv_firing_options fo = firing_opts_of_render(ropt);
	firing_run_params(hm, &fo, &r->fr);
	r->out_w = ropt->out_w; r->out_h = ropt->out_h;
	r->img_stride = (uint64_t)ropt->out_w * ropt->out_h * 4u;
	r->bytes_stride = (uint64_t)ropt->out_w * ropt->out_h;
	r->margin_m = o->margin_m;
	r->samples = o->samples;
	r->origin[0] = o->origin[0]; r->origin[1] = o->origin[1];
	r->origin_mode = o->origin_mode; r->line = o->line;
	memcpy(&r->pal[0], o->out_of_range, 4);
	memcpy(&r->pal[1], o->clear, 4);
	memcpy(&r->pal[2], o->blocked, 4);
	memcpy(&r->pal[3], o->los, 4);
}

extern "C" SMHV_API int smhv_batch_clearance_map(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *ropt,
                                                 const smhv_clearance_options *opt, void *d_bytes, void *stream) {
	if (!b) return fail(SMHV_E_INVALID, "batch_clearance_map: null batch");
	CTX_OPEN(b->ctx);
	int rc = check_render_options(ropt, hm, "batch_clearance_map");
	if (rc) return rc;
	rc = check_clearance_options(opt, true, "batch_clearance_map");
	if (rc) return rc;
	rc = check_frames(b, first, n, "batch_clearance_map");
	if (rc) return rc;
	rc = check_hm_device(hm, b->ctx->device, "batch_clearance_map", "batch");
	if (rc) return rc;
	const bool paint = (opt->flags & SMHV_CLEAR_PAINT) != 0u, bytes = (opt->flags & SMHV_CLEAR_BYTES) != 0u;
	if (bytes && !d_bytes) return fail(SMHV_E_INVALID, "batch_clearance_map: SMHV_CLEAR_BYTES and a null d_bytes");
	ClearMapRun r;
	clear_map_params(hm, ropt, opt, &r);
	hipStream_t s = (hipStream_t)stream;
	return window_pass_batch(b, first, n, hm, ropt, r, paint, "SMHV_CLEAR_PAINT", &b->d_clear_map, "clearance-map slab (%u frames)", &b->clear_map_hm, s,
	                         "batch_clearance_map", [&](ClearMapRun &part, uint32_t done, uint32_t k) -> int {
		part.bytes = bytes ? (uint8_t *)d_bytes + (size_t)done * r.bytes_stride : nullptr;
		HIPCHK(launch_clear_map(part, k, paint, bytes, s));
		return SMHV_OK;
	});
}

extern "C" SMHV_API int smhv_batch_read_clearance_map(smhv_batch *b, uint32_t first, uint32_t n, smhv_clearance_map_result *out) {
	return batch_read_slab(b, b ? b->d_clear_map : nullptr, sizeof(smhv_clearance_map_result), first, n, out, "batch_read_clearance_map",
	                       "this batch has computed no clearance map");
}

extern "C" SMHV_API int smhv_batch_clearance_map_ptr(smhv_batch *b, void **d_clearance_map) {
	return batch_slab_ptr(b, b ? b->d_clear_map : nullptr, d_clearance_map, "batch_clearance_map_ptr", "this batch has computed no clearance map");
}

// The per-call path (window_pass_per_call): the caller's image up, the kernel, the image, the bytes and the summary down.
extern "C" SMHV_API int smhv_clearance_map(smhv_ctx *c, const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_clearance_options *opt,
                                           const uint32_t minimap[4], uint8_t *rgba_inout, uint8_t *bytes, smhv_clearance_map_result *result) {
	if (!c) return fail(SMHV_E_INVALID, "clearance_map: null context");
	CTX_OPEN(c);
	if (!rgba_inout && !bytes) return fail(SMHV_E_INVALID, "clearance_map: neither an image nor a byte buffer");
	int rc = check_render_options(ropt, hm, "clearance_map");
	if (rc) return rc;
	rc = check_clearance_options(opt, true, "clearance_map");
	if (rc) return rc;
	if (opt->origin_mode != SMHV_REACH_ORIGIN_POINT)
		return fail(SMHV_E_INVALID, "clearance_map: origin mode %u (the per-call path takes SMHV_REACH_ORIGIN_POINT only)", opt->origin_mode);
	rc = check_hm_device(hm, c->device, "clearance_map", "context");
	if (rc) return rc;
	HIPCHK(hipSetDevice(c->device));
	ClearMapRun r;
	clear_map_params(hm, ropt, opt, &r);
	// [the summary, 256 bytes][the bytes][the image], each part on a 256-byte boundary
	StageLayout lay;
	lay.take(256u);
	const StagePart plane = lay.part(bytes, (size_t)r.bytes_stride), img = lay.part(rgba_inout, (size_t)r.img_stride);
	return window_pass_per_call(c, r, minimap, lay.total(), img, {plane, {result, 0, sizeof *result}}, [&](ClearMapRun &run, uint8_t *block, hipStream_t s) -> int {
		run.bytes = bytes ? block + plane.off : nullptr;
		HIPCHK(launch_clear_map(run, 1, rgba_inout != nullptr, bytes != nullptr, s));
		return SMHV_OK;
	});
}
