// smh_grid.inc -- the map grid: public entry points (smh_vision_hip.h, "map grid"; device code in smh_grid.hip, the rule in
// smh_grid.h).  Included at the end of smh_runtime.cpp.

extern "C" SMHV_API int smhv_grid_defaults(smhv_grid_options *opt) {
	static const uint8_t line[4][4] = {{0, 0, 0, 170}, {0, 0, 0, 110}, {0, 0, 0, 70}, {0, 0, 0, 45}}, label[4] = {0, 0, 0, 200};
	if (!opt) return fail(SMHV_E_INVALID, "grid_defaults: null options");
	memset(opt, 0, sizeof *opt);
	opt->size = sizeof *opt;
	opt->flags = SMHV_GRID_PAINT;
	opt->levels = 2u;
	opt->cell_m = 300.0;
	opt->min_px = 12.0;
	opt->label_min_px = 48.0;
	memcpy(opt->line, line, sizeof line);
	memcpy(opt->label, label, 4);
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_grid_ref_text(uint32_t col, uint32_t row1, const uint8_t *digits, uint32_t levels, char out[16]) {
	if (!out || col >= SMHV_GRID_MAX_COLS || row1 < 1u || row1 > SMHV_GRID_MAX_ROWS || levels > 3u || (levels && !digits))
		return fail(SMHV_E_INVALID, "grid_ref_text: column %u, row %u, %u levels", col, row1, levels);
	uint32_t d = 0u;
	for (uint32_t k = 0; k < levels; ++k) {
		if (digits[k] < 1u || digits[k] > 9u) return fail(SMHV_E_INVALID, "grid_ref_text: digit %u of level %u", digits[k], k + 1u);
		d |= (uint32_t)digits[k] << (8u * k);
	}
	grid_text(col, row1, d, levels, out);
	return SMHV_OK;
}

// what a call can get wrong in its grid options without the device being asked
static int check_grid_options(const smhv_grid_options *o, const char *what) {
	if (!o) return fail(SMHV_E_INVALID, "%s: null grid options", what);
	if (o->size != sizeof(smhv_grid_options)) return fail(SMHV_E_INVALID, "%s: smhv_grid_options.size %u != %zu", what, o->size, sizeof(smhv_grid_options));
	if (o->flags & ~(SMHV_GRID_PAINT | SMHV_GRID_BYTES | SMHV_GRID_CELLS)) return fail(SMHV_E_INVALID, "%s: unknown grid flags 0x%x", what, o->flags);
	if (!std::isfinite(o->cell_m) || o->cell_m <= 0.0) return fail(SMHV_E_INVALID, "%s: cell_m %g (finite, > 0)", what, o->cell_m);
	if (o->levels > 3u) return fail(SMHV_E_INVALID, "%s: %u levels (at most 3)", what, o->levels);
	if (!std::isfinite(o->origin_m[0]) || !std::isfinite(o->origin_m[1])) return fail(SMHV_E_INVALID, "%s: origin_m is not finite", what);
	if (!std::isfinite(o->min_px) || o->min_px < 0.0) return fail(SMHV_E_INVALID, "%s: min_px %g (finite, >= 0)", what, o->min_px);
	if (!std::isfinite(o->label_min_px)) return fail(SMHV_E_INVALID, "%s: label_min_px %g is not finite", what, o->label_min_px);
	return SMHV_OK;
}

// the launch arguments but for the frames' own pointers
static void grid_run_params(const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_grid_options *o, GridRun *r) {
	memset(r, 0, sizeof *r);
	const smhv_firing_options fo = firing_opts_of_render(ropt);
	firing_run_params(hm, &fo, &r->fr);
	r->out_w = ropt->out_w; r->out_h = ropt->out_h;
	r->img_stride = (uint64_t)ropt->out_w * ropt->out_h * 4u;
	r->plane_stride = (uint64_t)ropt->out_w * ropt->out_h;
	r->cell_m = o->cell_m; r->origin_m[0] = o->origin_m[0]; r->origin_m[1] = o->origin_m[1];
	r->min_px = o->min_px; r->label_min_px = o->label_min_px;
	r->levels = o->levels;
	for (int k = 0; k < 4; ++k) memcpy(&r->pal[k], o->line[k], 4);
	memcpy(&r->pal[4], o->label, 4);
}

// the checks smhv_batch_grid and smhv_batch_grid_refs share
static int check_batch_grid(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_grid_options *opt,
                            const char *what) {
	int rc = check_render_options(ropt, hm, what);
	if (rc) return rc;
	rc = check_grid_options(opt, what);
	if (rc) return rc;
	rc = check_frames(b, first, n, what);
	if (rc) return rc;
	return check_hm_device(hm, b->ctx->device, what, "batch");
}

extern "C" SMHV_API int smhv_batch_grid(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *ropt,
                                        const smhv_grid_options *opt, const smhv_grid_planes *planes, void *stream) {
	if (!b) return fail(SMHV_E_INVALID, "batch_grid: null batch");
	CTX_OPEN(b->ctx);
	int rc = check_batch_grid(b, first, n, hm, ropt, opt, "batch_grid");
	if (rc) return rc;
	const bool paint = (opt->flags & SMHV_GRID_PAINT) != 0u;
	uint8_t *d_bytes = nullptr;
	uint32_t *d_cells = nullptr;
	if (opt->flags & SMHV_GRID_BYTES) {
		if (!planes || !planes->bytes) return fail(SMHV_E_INVALID, "batch_grid: SMHV_GRID_BYTES and a null bytes plane");
		d_bytes = (uint8_t *)planes->bytes;
	}
	if (opt->flags & SMHV_GRID_CELLS) {
		if (!planes || !planes->cells) return fail(SMHV_E_INVALID, "batch_grid: SMHV_GRID_CELLS and a null cells plane");
		d_cells = (uint32_t *)planes->cells;
	}
	GridRun r;
	grid_run_params(hm, ropt, opt, &r);
	hipStream_t s = (hipStream_t)stream;
	return window_pass_batch(b, first, n, hm, ropt, r, paint, "SMHV_GRID_PAINT", &b->d_grid, "grid slab (%u frames)", &b->grid_hm, s, "batch_grid",
	                         [&](GridRun &part, uint32_t done, uint32_t k) -> int {
		part.bytes = d_bytes ? d_bytes + (size_t)done * r.plane_stride : nullptr;
		part.cells = d_cells ? d_cells + (size_t)done * r.plane_stride : nullptr;
		HIPCHK(launch_grid(part, k, paint, s));
		return SMHV_OK;
	});
}

extern "C" SMHV_API int smhv_batch_read_grid(smhv_batch *b, uint32_t first, uint32_t n, smhv_grid_result *out) {
	return batch_read_slab(b, b ? b->d_grid : nullptr, sizeof(smhv_grid_result), first, n, out, "batch_read_grid", "this batch has computed no grid");
}

extern "C" SMHV_API int smhv_batch_grid_ptr(smhv_batch *b, void **d_grid) {
	return batch_slab_ptr(b, b ? b->d_grid : nullptr, d_grid, "batch_grid_ptr", "this batch has computed no grid");
}

// The per-call path (window_pass_per_call): the caller's image up, the kernels, the image, the planes and the summary down.
extern "C" SMHV_API int smhv_grid_map(smhv_ctx *c, const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_grid_options *opt, const double *mpx,
                                      const uint32_t minimap[4], uint8_t *rgba_inout, uint8_t *bytes, uint32_t *cells, smhv_grid_result *result) {
	if (!c) return fail(SMHV_E_INVALID, "grid_map: null context");
	CTX_OPEN(c);
	if (!rgba_inout && !bytes && !cells && !result) return fail(SMHV_E_INVALID, "grid_map: no output");
	int rc = check_render_options(ropt, hm, "grid_map");
	if (rc) return rc;
	rc = check_grid_options(opt, "grid_map");
	if (rc) return rc;
	rc = check_hm_device(hm, c->device, "grid_map", "context");
	if (rc) return rc;
	HIPCHK(hipSetDevice(c->device));
	GridRun r;
	grid_run_params(hm, ropt, opt, &r);
	r.has_mpx = mpx ? 1u : 0u;
	r.mpx = mpx ? *mpx : 0.0;
	// [the summary, 256 bytes][the flag bytes][the cell words][the image], each part on a 256-byte boundary
	StageLayout lay;
	lay.take(256u);
	const size_t px = (size_t)r.plane_stride;
	const StagePart pb = lay.part(bytes, px), pc = lay.part(cells, px * sizeof(uint32_t)), img = lay.part(rgba_inout, (size_t)r.img_stride);
	return window_pass_per_call(c, r, minimap, lay.total(), img, {pb, pc, {result, 0, sizeof *result}}, [&](GridRun &run, uint8_t *block, hipStream_t s) -> int {
		run.bytes = bytes ? block + pb.off : nullptr;
		run.cells = cells ? (uint32_t *)(block + pc.off) : nullptr;
		HIPCHK(launch_grid(run, 1, rgba_inout != nullptr, s));
		return SMHV_OK;
	});
}

// ---- the references of the line ends
extern "C" SMHV_API int smhv_batch_grid_refs(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *ropt,
                                             const smhv_grid_options *opt, void *stream) {
	if (!b) return fail(SMHV_E_INVALID, "batch_grid_refs: null batch");
	CTX_OPEN(b->ctx);
	int rc = check_batch_grid(b, first, n, hm, ropt, opt, "batch_grid_refs");
	if (rc) return rc;
	HIPCHK(hipSetDevice(b->ctx->device));
	rc = first_use_slabs(b, "grid references slab (%u frames)", {{(void **)&b->d_grid_refs, sizeof(smhv_grid_refs_result) * (size_t)b->max_frames, 0}});
	if (rc) return rc;
	hipStream_t s = (hipStream_t)stream;
	GridRun r;
	grid_run_params(hm, ropt, opt, &r);
	r.aux = b->d_aux + first;
	r.res = b->d_results + first;
	r.refs = b->d_grid_refs + first;
	HIPCHK(launch_grid_refs(r, n, s));
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_batch_read_grid_refs(smhv_batch *b, uint32_t first, uint32_t n, smhv_grid_refs_result *out) {
	return batch_read_slab(b, b ? b->d_grid_refs : nullptr, sizeof(smhv_grid_refs_result), first, n, out, "batch_read_grid_refs",
	                       "this batch has computed no grid references");
}

extern "C" SMHV_API int smhv_batch_grid_refs_ptr(smhv_batch *b, void **d_grid_refs) {
	return batch_slab_ptr(b, b ? b->d_grid_refs : nullptr, d_grid_refs, "batch_grid_refs_ptr", "this batch has computed no grid references");
}

// The per-call form: the lines up, the kernel, the references down, through the context's pinned block.
extern "C" SMHV_API int smhv_grid_refs(smhv_ctx *c, const smhv_line *lines, uint32_t n, const double *mpx, const uint32_t minimap[4], const smhv_heightmap *hm,
                                       const smhv_render_options *ropt, const smhv_grid_options *opt, smhv_grid_ref *out) {
	if (!c || (n && (!lines || !out))) return fail(SMHV_E_INVALID, "grid_refs: null argument");
	CTX_OPEN(c);
	int rc = check_render_options(ropt, hm, "grid_refs");
	if (rc) return rc;
	rc = check_grid_options(opt, "grid_refs");
	if (rc) return rc;
	if (n == 0) return SMHV_OK;
	if (n > 0x3FFFFFFFu) return fail(SMHV_E_INVALID, "grid_refs: %u lines", n);
	rc = check_hm_device(hm, c->device, "grid_refs", "context");
	if (rc) return rc;
	HIPCHK(hipSetDevice(c->device));
	GridRun r;
	grid_run_params(hm, ropt, opt, &r);
	r.per_call = 1u; r.n_lines = n;
	r.has_mpx = mpx ? 1u : 0u;
	r.mpx = mpx ? *mpx : 0.0;
	r.has_mm = minimap ? 1u : 0u;
	if (minimap) memcpy(r.mm, minimap, sizeof r.mm);
	// [the lines][the references], each part on a 256-byte boundary
	StageLayout lay;
	const size_t in_bytes = sizeof(smhv_line) * (size_t)n, out_bytes = sizeof(smhv_grid_ref) * 2u * (size_t)n;
	lay.take(in_bytes);
	const size_t out_off = lay.take(out_bytes);
	std::lock_guard<std::mutex> lk(c->fire_mu);
	rc = ctx_stage_reserve(c, lay.total());
	if (rc) return rc;
	r.lines = (const smhv_line *)c->d_fire;
	r.refs_out = (smhv_grid_ref *)(c->d_fire + out_off);
	memcpy(c->h_fire, lines, in_bytes);
	HIPCHK(hipMemcpyAsync(c->d_fire, c->h_fire, in_bytes, hipMemcpyHostToDevice, c->s_main));
	HIPCHK(launch_grid_refs(r, 1, c->s_main));
	HIPCHK(hipMemcpyAsync(c->h_fire + out_off, c->d_fire + out_off, out_bytes, hipMemcpyDeviceToHost, c->s_main));
	HIPCHK(wait_stream(c->s_main));
	memcpy(out, c->h_fire + out_off, out_bytes);
	return SMHV_OK;
}
