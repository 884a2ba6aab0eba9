// smh_ballistics.inc -- ballistics: public entry points (smh_vision_hip.h, "ballistics"; device code in smh_ballistics.hip, the rule in
// smh_ballistics.h).  Included at the end of smh_runtime.cpp.

// ---- host only: the weapon and one solution
extern "C" SMHV_API int smhv_weapon_defaults(smhv_weapon *w) {
	if (!w) return fail(SMHV_E_INVALID, "weapon_defaults: null weapon");
	memset(w, 0, sizeof *w);
	w->size = sizeof *w;
	w->arc = SMHV_ARC_HIGH;
	w->unit = SMHV_ANGLE_MILS6400;
	w->velocity = 109.890938;                                      // squadex::milliradians: VELOCITY, GRAVITY
	w->gravity = 9.8;
	w->elev_min = 0.0; w->elev_max = 1600.0;                       // (a quarter turn: no limit)
	return SMHV_OK;
}

// what a call can get wrong in its weapon without the device being asked
static int check_weapon(const smhv_weapon *w, const char *what) {
	if (!w) return fail(SMHV_E_INVALID, "%s: null weapon", what);
	if (w->size != sizeof(smhv_weapon)) return fail(SMHV_E_INVALID, "%s: smhv_weapon.size %u != %zu", what, w->size, sizeof(smhv_weapon));
	if (!weapon_ok(w))
		return fail(SMHV_E_INVALID, "%s: weapon: arc %u, unit %u, velocity %g, gravity %g (finite, > 0), limits %g .. %g (finite, in order), range_min %g, dispersion %g (finite, >= 0)",
		            what, w->arc, w->unit, w->velocity, w->gravity, w->elev_min, w->elev_max, w->range_min, w->dispersion);
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_weapon_check(const smhv_weapon *w) { return check_weapon(w, "weapon_check"); }

extern "C" SMHV_API int smhv_weapon_thresholds(const smhv_weapon *w, smhv_weapon_rule *out) {
	if (!out) return fail(SMHV_E_INVALID, "weapon_thresholds: null argument");
	const int rc = check_weapon(w, "weapon_thresholds");
	if (rc) return rc;
	weapon_rule(w, out);
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_ballistic_solve(const smhv_weapon *w, double meters, double alt, smhv_ballistic_solution *out) {
	if (!out) return fail(SMHV_E_INVALID, "ballistic_solve: null argument");
	const int rc = check_weapon(w, "ballistic_solve");
	if (rc) return rc;
	smhv_weapon_rule rule;
	weapon_rule(w, &rule);
	*out = bal_solve(rule, meters, alt, 0u);
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_ballistic_defaults(smhv_ballistic_options *opt) {
	static const uint8_t pal[12][4] = {{200, 30, 30, 96}, {120, 120, 120, 96}, {150, 60, 160, 96}, {90, 60, 200, 96},
	                                   {40, 90, 255, 72}, {0, 170, 255, 72}, {0, 220, 200, 72}, {0, 230, 110, 72},
	                                   {120, 235, 0, 72}, {220, 230, 0, 72}, {255, 180, 0, 72}, {255, 120, 40, 72}};
	static const uint8_t iso[4] = {255, 255, 255, 160};
	if (!opt) return fail(SMHV_E_INVALID, "ballistic_defaults: null options");
	memset(opt, 0, sizeof *opt);
	opt->size = sizeof *opt;
	opt->flags = SMHV_BMAP_PAINT;
	opt->origin_mode = SMHV_REACH_ORIGIN_POINT;
	memcpy(opt->pal, pal, sizeof pal);
	memcpy(opt->iso, iso, 4);
	return SMHV_OK;
}

// what a call can get wrong in its map options without the device being asked
static int check_ballistic_options(const smhv_ballistic_options *o, const char *what) {
	if (!o) return fail(SMHV_E_INVALID, "%s: null ballistic options", what);
	if (o->size != sizeof(smhv_ballistic_options)) return fail(SMHV_E_INVALID, "%s: smhv_ballistic_options.size %u != %zu", what, o->size, sizeof(smhv_ballistic_options));
	if (o->flags & ~(SMHV_BMAP_PAINT | SMHV_BMAP_CLASSES | SMHV_BMAP_TOF)) return fail(SMHV_E_INVALID, "%s: unknown ballistic flags 0x%x", what, o->flags);
	if (o->origin_mode > SMHV_REACH_ORIGIN_LINE_P1) return fail(SMHV_E_INVALID, "%s: origin mode %u", what, o->origin_mode);
	if (o->origin_mode != SMHV_REACH_ORIGIN_POINT && o->line >= (uint32_t)SMHV_MAX_LINES)
		return fail(SMHV_E_INVALID, "%s: line %u (a record holds %u)", what, o->line, (unsigned)SMHV_MAX_LINES);
	if (!std::isfinite(o->iso_s) || o->iso_s < 0.0) return fail(SMHV_E_INVALID, "%s: iso_s %g (finite, >= 0)", what, o->iso_s);
	return SMHV_OK;
}

// ---- the lines
extern "C" SMHV_API int smhv_batch_ballistics(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_firing_options *fopt,
                                              const smhv_weapon *weapon, void *stream) {
	if (!b) return fail(SMHV_E_INVALID, "batch_ballistics: null batch");
	CTX_OPEN(b->ctx);
	int rc = check_firing_options(fopt);
	if (rc) return rc;
	rc = check_weapon(weapon, "batch_ballistics");
	if (rc) return rc;
	rc = check_frames(b, first, n, "batch_ballistics");
	if (rc) return rc;
	rc = check_hm_device(hm, b->ctx->device, "batch_ballistics", "batch");
	if (rc) return rc;
	HIPCHK(hipSetDevice(b->ctx->device));
	rc = first_use_slabs(b, "ballistics slab (%u frames)", {{(void **)&b->d_bal, sizeof(smhv_ballistic_result) * (size_t)b->max_frames, 0}});
	if (rc) return rc;
	hipStream_t s = (hipStream_t)stream;
	hm_rebind(&b->bal_hm, hm);                                     // the batch's reference of the heightmap its enqueued call reads
	const smhv_firing_options fo = firing_opts(fopt);
	BalLinesRun r;
	memset(&r, 0, sizeof r);
	firing_run_params(hm, &fo, &r.fr);
	weapon_rule(weapon, &r.w);
	return for_each_launch(n, [&](uint32_t done, uint32_t k) -> int {
		BalLinesRun part = r;
		part.res = b->d_results + first + done;
		part.out = b->d_bal + first + done;
		HIPCHK(launch_ballistic_lines(part, k, s));
		return SMHV_OK;
	});
}

extern "C" SMHV_API int smhv_batch_read_ballistics(smhv_batch *b, uint32_t first, uint32_t n, smhv_ballistic_result *out) {
	return batch_read_slab(b, b ? b->d_bal : nullptr, sizeof(smhv_ballistic_result), first, n, out, "batch_read_ballistics", "this batch has computed no ballistics");
}

extern "C" SMHV_API int smhv_batch_ballistics_ptr(smhv_batch *b, void **d_ballistics) {
	return batch_slab_ptr(b, b ? b->d_bal : nullptr, d_ballistics, "batch_ballistics_ptr", "this batch has computed no ballistics");
}

// The per-call path: the lines up, the kernel, the records down, through the context's pinned block.
extern "C" SMHV_API int smhv_ballistic_lines(smhv_ctx *c, const smhv_line *lines, uint32_t n, const double *mpx, const uint32_t minimap[4], const smhv_heightmap *hm,
                                             const smhv_firing_options *fopt, const smhv_weapon *weapon, smhv_ballistic *out) {
	if (!c || (n && (!lines || !out))) return fail(SMHV_E_INVALID, "ballistic_lines: null argument");
	CTX_OPEN(c);
	int rc = check_firing_options(fopt);
	if (rc) return rc;
	rc = check_weapon(weapon, "ballistic_lines");
	if (rc) return rc;
	if (n == 0) return SMHV_OK;
	rc = check_hm_device(hm, c->device, "ballistic_lines", "context");
	if (rc) return rc;
	HIPCHK(hipSetDevice(c->device));
	const smhv_firing_options fo = firing_opts(fopt);
	BalLinesRun r;
	memset(&r, 0, sizeof r);
	firing_run_params(hm, &fo, &r.fr);
	weapon_rule(weapon, &r.w);
	r.per_call = 1u; r.n_lines = n;
	r.has_mpx = mpx ? 1u : 0u; r.mpx = mpx ? *mpx : 0.0;
	r.has_mm = minimap ? 1u : 0u;
	if (minimap) memcpy(r.mm, minimap, sizeof r.mm);
	// [the lines][the records], each part on a 256-byte boundary
	StageLayout lay;
	const size_t in_bytes = sizeof(smhv_line) * (size_t)n;
	lay.take(in_bytes);
	const StagePart rec = lay.part(out, sizeof(smhv_ballistic) * (size_t)n);
	std::lock_guard<std::mutex> lk(c->fire_mu);
	rc = ctx_stage_reserve(c, lay.total());
	if (rc) return rc;
	r.lines = (const smhv_line *)c->d_fire;
	r.out_lines = (smhv_ballistic *)(c->d_fire + rec.off);
	memcpy(c->h_fire, lines, in_bytes);
	HIPCHK(hipMemcpyAsync(c->d_fire, c->h_fire, in_bytes, hipMemcpyHostToDevice, c->s_main));
	HIPCHK(launch_ballistic_lines(r, 1, c->s_main));
	HIPCHK(hipMemcpyAsync(c->h_fire + rec.off, c->d_fire + rec.off, rec.len, hipMemcpyDeviceToHost, c->s_main));
	HIPCHK(wait_stream(c->s_main));
	memcpy(out, c->h_fire + rec.off, rec.len);
	return SMHV_OK;
}

// ---- the map
// the launch arguments but for the frames' own pointers
static void ballistic_map_params(const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_weapon *w, const smhv_ballistic_options *o, BalMapRun *r) {
	memset(r, 0, sizeof *r);
	const smhv_firing_options fo = firing_opts_of_render(ropt);
	firing_run_params(hm, &fo, &r->fr);
	weapon_rule(w, &r->w);
	r->out_w = ropt->out_w; r->out_h = ropt->out_h;
	r->img_stride = (uint64_t)ropt->out_w * ropt->out_h * 4u;
	r->plane_stride = (uint64_t)ropt->out_w * ropt->out_h;
	r->iso_s = o->iso_s;
	r->origin[0] = o->origin[0]; r->origin[1] = o->origin[1];
	r->origin_mode = o->origin_mode; r->line = o->line;
	memcpy(&r->pal[0], o->pal, 48);
	memcpy(&r->pal[12], o->iso, 4);
}

extern "C" SMHV_API int smhv_batch_ballistic_map(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *ropt,
                                                 const smhv_weapon *weapon, const smhv_ballistic_options *opt, const smhv_ballistic_planes *planes, void *stream) {
	if (!b) return fail(SMHV_E_INVALID, "batch_ballistic_map: null batch");
	CTX_OPEN(b->ctx);
	int rc = check_render_options(ropt, hm, "batch_ballistic_map");
	if (rc) return rc;
	rc = check_weapon(weapon, "batch_ballistic_map");
	if (rc) return rc;
	rc = check_ballistic_options(opt, "batch_ballistic_map");
	if (rc) return rc;
	rc = check_frames(b, first, n, "batch_ballistic_map");
	if (rc) return rc;
	rc = check_hm_device(hm, b->ctx->device, "batch_ballistic_map", "batch");
	if (rc) return rc;
	const bool paint = (opt->flags & SMHV_BMAP_PAINT) != 0u;
	uint8_t *d_cls = nullptr;
	float *d_tof = nullptr;
	if (opt->flags & SMHV_BMAP_CLASSES) {
		if (!planes || !planes->classes) return fail(SMHV_E_INVALID, "batch_ballistic_map: SMHV_BMAP_CLASSES and a null classes plane");
		d_cls = (uint8_t *)planes->classes;
	}
	if (opt->flags & SMHV_BMAP_TOF) {
		if (!planes || !planes->tof) return fail(SMHV_E_INVALID, "batch_ballistic_map: SMHV_BMAP_TOF and a null tof plane");
		d_tof = (float *)planes->tof;
	}
	BalMapRun r;
	ballistic_map_params(hm, ropt, weapon, opt, &r);
	hipStream_t s = (hipStream_t)stream;
	return window_pass_batch(b, first, n, hm, ropt, r, paint, "SMHV_BMAP_PAINT", &b->d_bal_map, "ballistic-map slab (%u frames)", &b->bal_map_hm, s,
	                         "batch_ballistic_map", [&](BalMapRun &part, uint32_t done, uint32_t k) -> int {
		part.cls = d_cls ? d_cls + (size_t)done * r.plane_stride : nullptr;
		part.tof = d_tof ? d_tof + (size_t)done * r.plane_stride : nullptr;
		HIPCHK(launch_ballistic_map(part, k, paint, s));
		return SMHV_OK;
	});
}

extern "C" SMHV_API int smhv_batch_read_ballistic_map(smhv_batch *b, uint32_t first, uint32_t n, smhv_ballistic_map_result *out) {
	return batch_read_slab(b, b ? b->d_bal_map : nullptr, sizeof(smhv_ballistic_map_result), first, n, out, "batch_read_ballistic_map",
	                       "this batch has computed no ballistic map");
}

extern "C" SMHV_API int smhv_batch_ballistic_map_ptr(smhv_batch *b, void **d_ballistic_map) {
	return batch_slab_ptr(b, b ? b->d_bal_map : nullptr, d_ballistic_map, "batch_ballistic_map_ptr", "this batch has computed no ballistic map");
}

// The per-call path (window_pass_per_call): the caller's image up, the kernels, the image, the planes and the summary down.
extern "C" SMHV_API int smhv_ballistic_map(smhv_ctx *c, const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_weapon *weapon,
                                           const smhv_ballistic_options *opt, const double *mpx, const uint32_t minimap[4], uint8_t *rgba_inout, uint8_t *classes,
                                           float *tof, smhv_ballistic_map_result *result) {
	if (!c) return fail(SMHV_E_INVALID, "ballistic_map: null context");
	CTX_OPEN(c);
	if (!rgba_inout && !classes && !tof && !result) return fail(SMHV_E_INVALID, "ballistic_map: no output");
	int rc = check_render_options(ropt, hm, "ballistic_map");
	if (rc) return rc;
	rc = check_weapon(weapon, "ballistic_map");
	if (rc) return rc;
	rc = check_ballistic_options(opt, "ballistic_map");
	if (rc) return rc;
	if (opt->origin_mode != SMHV_REACH_ORIGIN_POINT)
		return fail(SMHV_E_INVALID, "ballistic_map: origin mode %u (the per-call path takes SMHV_REACH_ORIGIN_POINT only)", opt->origin_mode);
	rc = check_hm_device(hm, c->device, "ballistic_map", "context");
	if (rc) return rc;
	HIPCHK(hipSetDevice(c->device));
	BalMapRun r;
	ballistic_map_params(hm, ropt, weapon, opt, &r);
	r.has_mpx = mpx ? 1u : 0u; r.mpx = mpx ? *mpx : 0.0;
	// [the summary, 256 bytes][the classes][the times][the image], each part on a 256-byte boundary
	StageLayout lay;
	lay.take(256u);
	const size_t px = (size_t)r.plane_stride;
	const StagePart pc = lay.part(classes, px), pt = lay.part(tof, px * sizeof(float)), img = lay.part(rgba_inout, (size_t)r.img_stride);
	return window_pass_per_call(c, r, minimap, lay.total(), img, {pc, pt, {result, 0, sizeof *result}}, [&](BalMapRun &run, uint8_t *block, hipStream_t s) -> int {
		run.cls = classes ? block + pc.off : nullptr;
		run.tof = tof ? (float *)(block + pt.off) : nullptr;
		HIPCHK(launch_ballistic_map(run, 1, rgba_inout != nullptr, s));
		return SMHV_OK;
	});
}
