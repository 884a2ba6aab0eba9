// smh_balclear.inc -- ballistic clearance: public entry points (smh_vision_hip.h, "ballistic clearance"; device code in smh_balclear.hip,
// the per-arc steps of the rule in smh_ballistics.h).  Included at the end of smh_runtime.cpp, behind smh_ballistics.inc (check_weapon).

extern "C" SMHV_API int smhv_ballistic_clearance_defaults(smhv_ballistic_clearance_options *opt) {
	static const uint8_t blocked[4] = {230, 40, 40, 110}, sw[4] = {240, 190, 40, 110}, los[4] = {0, 0, 0, 70};
	if (!opt) return fail(SMHV_E_INVALID, "ballistic_clearance_defaults: null options");
	memset(opt, 0, sizeof *opt);
	opt->size = sizeof *opt;
	opt->flags = SMHV_BCLR_PAINT;
	opt->samples = 64u;
	opt->origin_mode = SMHV_REACH_ORIGIN_POINT;
	memcpy(opt->pal[SMHV_BCLR_BLOCKED - 1u], blocked, 4);
	memcpy(opt->switch_arc, sw, 4);
	memcpy(opt->los, los, 4);
	return SMHV_OK;
}

// what a call can get wrong in its options without the device being asked
static int check_ballistic_clearance_options(const smhv_ballistic_clearance_options *o, const char *what) {
	if (!o) return fail(SMHV_E_INVALID, "%s: null ballistic clearance options", what);
	if (o->size != sizeof(smhv_ballistic_clearance_options))
		return fail(SMHV_E_INVALID, "%s: smhv_ballistic_clearance_options.size %u != %zu", what, o->size, sizeof(smhv_ballistic_clearance_options));
	if (o->flags & ~(SMHV_BCLR_PAINT | SMHV_BCLR_BYTES | SMHV_BCLR_MARGIN)) return fail(SMHV_E_INVALID, "%s: unknown ballistic clearance flags 0x%x", what, o->flags);
	if (o->samples == 0u || o->samples > SMHV_CLEAR_MAX_SAMPLES)
		return fail(SMHV_E_INVALID, "%s: %u samples (1 .. %u)", what, o->samples, (unsigned)SMHV_CLEAR_MAX_SAMPLES);
	if (!std::isfinite(o->margin_m) || o->margin_m < 0.0) return fail(SMHV_E_INVALID, "%s: margin_m %g (finite, >= 0)", what, o->margin_m);
	if (o->origin_mode > SMHV_REACH_ORIGIN_LINE_P1) return fail(SMHV_E_INVALID, "%s: origin mode %u", what, o->origin_mode);
	if (o->origin_mode != SMHV_REACH_ORIGIN_POINT && o->line >= (uint32_t)SMHV_MAX_LINES)
		return fail(SMHV_E_INVALID, "%s: line %u (a record holds %u)", what, o->line, (unsigned)SMHV_MAX_LINES);
	if (o->reserved0 || o->reserved[0] || o->reserved[1] || o->reserved[2] || o->reserved[3])
		return fail(SMHV_E_INVALID, "%s: a reserved word of smhv_ballistic_clearance_options is not 0", what);
	return SMHV_OK;
}

// host only, for the tests: the options check on its own
extern "C" SMHV_API int smhv_ballistic_clearance_check(const smhv_ballistic_clearance_options *opt) {
	return check_ballistic_clearance_options(opt, "ballistic_clearance_check");
}

// ---- the lines
extern "C" SMHV_API int smhv_batch_ballistic_clearance(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_firing_options *fopt,
                                                       const smhv_weapon *weapon, const smhv_ballistic_clearance_options *opt, void *stream) {
	if (!b) return fail(SMHV_E_INVALID, "batch_ballistic_clearance: null batch");
	CTX_OPEN(b->ctx);
	int rc = check_firing_options(fopt);
	if (rc) return rc;
	rc = check_weapon(weapon, "batch_ballistic_clearance");
	if (rc) return rc;
	rc = check_ballistic_clearance_options(opt, "batch_ballistic_clearance");
	if (rc) return rc;
	rc = check_frames(b, first, n, "batch_ballistic_clearance");
	if (rc) return rc;
	rc = check_hm_device(hm, b->ctx->device, "batch_ballistic_clearance", "batch");
	if (rc) return rc;
	HIPCHK(hipSetDevice(b->ctx->device));
	rc = first_use_slabs(b, "ballistic-clearance slab (%u frames)", {{(void **)&b->d_bclear, sizeof(smhv_ballistic_clearance_result) * (size_t)b->max_frames, 0}});
	if (rc) return rc;
	hipStream_t s = (hipStream_t)stream;
	hm_rebind(&b->bclear_hm, hm);                                  // the batch's reference of the heightmap its enqueued call reads
	const smhv_firing_options fo = firing_opts(fopt);
	BalClearLinesRun r;
	memset(&r, 0, sizeof r);
	firing_run_params(hm, &fo, &r.fr);
	weapon_rule(weapon, &r.w);
	r.margin_m = opt->margin_m;
	r.samples = opt->samples;
	return for_each_launch(n, [&](uint32_t done, uint32_t k) -> int {
		BalClearLinesRun part = r;
		part.res = b->d_results + first + done;
		part.out = b->d_bclear + first + done;
		HIPCHK(launch_bclear_lines(part, k, s));
		return SMHV_OK;
	});
}

extern "C" SMHV_API int smhv_batch_read_ballistic_clearance(smhv_batch *b, uint32_t first, uint32_t n, smhv_ballistic_clearance_result *out) {
	return batch_read_slab(b, b ? b->d_bclear : nullptr, sizeof(smhv_ballistic_clearance_result), first, n, out, "batch_read_ballistic_clearance",
	                       "this batch has computed no ballistic clearance");
}

extern "C" SMHV_API int smhv_batch_ballistic_clearance_ptr(smhv_batch *b, void **d_ballistic_clearance) {
	return batch_slab_ptr(b, b ? b->d_bclear : nullptr, d_ballistic_clearance, "batch_ballistic_clearance_ptr", "this batch has computed no ballistic clearance");
}

// The per-call path: the lines up, the kernel, the records down, through the context's pinned block.
extern "C" SMHV_API int smhv_ballistic_clearance_lines(smhv_ctx *c, const smhv_line *lines, uint32_t n, const uint32_t minimap[4], const smhv_heightmap *hm,
                                                       const smhv_firing_options *fopt, const smhv_weapon *weapon, const smhv_ballistic_clearance_options *opt,
                                                       smhv_ballistic_clearance *out) {
	if (!c || (n && (!lines || !out))) return fail(SMHV_E_INVALID, "ballistic_clearance_lines: null argument");
	CTX_OPEN(c);
	int rc = check_firing_options(fopt);
	if (rc) return rc;
	rc = check_weapon(weapon, "ballistic_clearance_lines");
	if (rc) return rc;
	rc = check_ballistic_clearance_options(opt, "ballistic_clearance_lines");
	if (rc) return rc;
	if (n == 0) return SMHV_OK;
	rc = check_hm_device(hm, c->device, "ballistic_clearance_lines", "context");
	if (rc) return rc;
	HIPCHK(hipSetDevice(c->device));
	const smhv_firing_options fo = firing_opts(fopt);
	BalClearLinesRun r;
	memset(&r, 0, sizeof r);
	firing_run_params(hm, &fo, &r.fr);
	weapon_rule(weapon, &r.w);
	r.margin_m = opt->margin_m;
	r.samples = opt->samples;
	r.per_call = 1u; r.n_lines = n;
	r.has_mm = minimap ? 1u : 0u;
	if (minimap) memcpy(r.mm, minimap, sizeof r.mm);
	// [the lines][the records], each part on a 256-byte boundary
	StageLayout lay;
	const size_t in_bytes = sizeof(smhv_line) * (size_t)n;
	lay.take(in_bytes);
	const StagePart rec = lay.part(out, sizeof(smhv_ballistic_clearance) * (size_t)n);
	std::lock_guard<std::mutex> lk(c->fire_mu);
	rc = ctx_stage_reserve(c, lay.total());
	if (rc) return rc;
	r.lines = (const smhv_line *)c->d_fire;
	r.out_lines = (smhv_ballistic_clearance *)(c->d_fire + rec.off);
	memcpy(c->h_fire, lines, in_bytes);
	HIPCHK(hipMemcpyAsync(c->d_fire, c->h_fire, in_bytes, hipMemcpyHostToDevice, c->s_main));
	HIPCHK(launch_bclear_lines(r, 1, c->s_main));
	HIPCHK(hipMemcpyAsync(c->h_fire + rec.off, c->d_fire + rec.off, rec.len, hipMemcpyDeviceToHost, c->s_main));
	HIPCHK(wait_stream(c->s_main));
	memcpy(out, c->h_fire + rec.off, rec.len);
	return SMHV_OK;
}

// ---- the map
// the launch arguments but for the frames' own pointers
static void bclear_map_params(const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_weapon *w, const smhv_ballistic_clearance_options *o,
                              BalClearMapRun *r) {
	memset(r, 0, sizeof *r);
	const smhv_firing_options fo = firing_opts_of_render(ropt);
	firing_run_params(hm, &fo, &r->fr);
	weapon_rule(w, &r->w);
	r->out_w = ropt->out_w; r->out_h = ropt->out_h;
	r->img_stride = (uint64_t)ropt->out_w * ropt->out_h * 4u;
	r->plane_stride = (uint64_t)ropt->out_w * ropt->out_h;
	r->margin_m = o->margin_m;
	r->samples = o->samples;
	r->origin[0] = o->origin[0]; r->origin[1] = o->origin[1];
	r->origin_mode = o->origin_mode; r->line = o->line;
	memcpy(&r->pal[0], o->pal, 16);
	memcpy(&r->pal[4], o->switch_arc, 4);
	memcpy(&r->pal[5], o->los, 4);
}

extern "C" SMHV_API int smhv_batch_ballistic_clearance_map(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *ropt,
                                                           const smhv_weapon *weapon, const smhv_ballistic_clearance_options *opt,
                                                           const smhv_ballistic_clearance_planes *planes, void *stream) {
	if (!b) return fail(SMHV_E_INVALID, "batch_ballistic_clearance_map: null batch");
	CTX_OPEN(b->ctx);
	int rc = check_render_options(ropt, hm, "batch_ballistic_clearance_map");
	if (rc) return rc;
	rc = check_weapon(weapon, "batch_ballistic_clearance_map");
	if (rc) return rc;
	rc = check_ballistic_clearance_options(opt, "batch_ballistic_clearance_map");
	if (rc) return rc;
	rc = check_frames(b, first, n, "batch_ballistic_clearance_map");
	if (rc) return rc;
	rc = check_hm_device(hm, b->ctx->device, "batch_ballistic_clearance_map", "batch");
	if (rc) return rc;
	const bool paint = (opt->flags & SMHV_BCLR_PAINT) != 0u;
	uint8_t *d_bytes = nullptr;
	float *d_margin = nullptr;
	if (opt->flags & SMHV_BCLR_BYTES) {
		if (!planes || !planes->bytes) return fail(SMHV_E_INVALID, "batch_ballistic_clearance_map: SMHV_BCLR_BYTES and a null bytes plane");
		d_bytes = (uint8_t *)planes->bytes;
	}
	if (opt->flags & SMHV_BCLR_MARGIN) {
		if (!planes || !planes->margin) return fail(SMHV_E_INVALID, "batch_ballistic_clearance_map: SMHV_BCLR_MARGIN and a null margin plane");
		d_margin = (float *)planes->margin;
	}
	BalClearMapRun r;
	bclear_map_params(hm, ropt, weapon, opt, &r);
	hipStream_t s = (hipStream_t)stream;
	return window_pass_batch(b, first, n, hm, ropt, r, paint, "SMHV_BCLR_PAINT", &b->d_bclear_map, "ballistic-clearance-map slab (%u frames)", &b->bclear_map_hm, s,
	                         "batch_ballistic_clearance_map", [&](BalClearMapRun &part, uint32_t done, uint32_t k) -> int {
		part.bytes = d_bytes ? d_bytes + (size_t)done * r.plane_stride : nullptr;
		part.margin = d_margin ? d_margin + (size_t)done * r.plane_stride : nullptr;
		HIPCHK(launch_bclear_map(part, k, paint, s));
		return SMHV_OK;
	});
}

extern "C" SMHV_API int smhv_batch_read_ballistic_clearance_map(smhv_batch *b, uint32_t first, uint32_t n, smhv_ballistic_clearance_map_result *out) {
	return batch_read_slab(b, b ? b->d_bclear_map : nullptr, sizeof(smhv_ballistic_clearance_map_result), first, n, out, "batch_read_ballistic_clearance_map",
	                       "this batch has computed no ballistic clearance map");
}

extern "C" SMHV_API int smhv_batch_ballistic_clearance_map_ptr(smhv_batch *b, void **d_ballistic_clearance_map) {
	return batch_slab_ptr(b, b ? b->d_bclear_map : nullptr, d_ballistic_clearance_map, "batch_ballistic_clearance_map_ptr",
	                      "this batch has computed no ballistic clearance map");
}

// The per-call path (window_pass_per_call): the caller's image up, the kernel, the image, the planes and the summary down.
extern "C" SMHV_API int smhv_ballistic_clearance_map(smhv_ctx *c, const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_weapon *weapon,
                                                     const smhv_ballistic_clearance_options *opt, const uint32_t minimap[4], uint8_t *rgba_inout, uint8_t *bytes,
                                                     float *margin, smhv_ballistic_clearance_map_result *result) {
	if (!c) return fail(SMHV_E_INVALID, "ballistic_clearance_map: null context");
	CTX_OPEN(c);
	if (!rgba_inout && !bytes && !margin && !result) return fail(SMHV_E_INVALID, "ballistic_clearance_map: no output");
	int rc = check_render_options(ropt, hm, "ballistic_clearance_map");
	if (rc) return rc;
	rc = check_weapon(weapon, "ballistic_clearance_map");
	if (rc) return rc;
	rc = check_ballistic_clearance_options(opt, "ballistic_clearance_map");
	if (rc) return rc;
	if (opt->origin_mode != SMHV_REACH_ORIGIN_POINT)
		return fail(SMHV_E_INVALID, "ballistic_clearance_map: origin mode %u (the per-call path takes SMHV_REACH_ORIGIN_POINT only)", opt->origin_mode);
	rc = check_hm_device(hm, c->device, "ballistic_clearance_map", "context");
	if (rc) return rc;
	HIPCHK(hipSetDevice(c->device));
	BalClearMapRun r;
	bclear_map_params(hm, ropt, weapon, opt, &r);
	// [the summary, 256 bytes][the bytes][the margins][the image], each part on a 256-byte boundary
	StageLayout lay;
	lay.take(256u);
	const size_t px = (size_t)r.plane_stride;
	const StagePart pb = lay.part(bytes, px), pm = lay.part(margin, px * sizeof(float)), img = lay.part(rgba_inout, (size_t)r.img_stride);
	return window_pass_per_call(c, r, minimap, lay.total(), img, {pb, pm, {result, 0, sizeof *result}}, [&](BalClearMapRun &run, uint8_t *block, hipStream_t s) -> int {
		run.bytes = bytes ? block + pb.off : nullptr;
		run.margin = margin ? (float *)(block + pm.off) : nullptr;
		HIPCHK(launch_bclear_map(run, 1, rgba_inout != nullptr, s));
		return SMHV_OK;
	});
}
