// smh_debugtext.inc -- the vision debugger and the Debug menu's text of the map view: public entry points (smh_vision_hip.h, "map
// view: debug text and the vision debugger"; device code in smh_debugtext.hip).  Included at the end of smh_runtime.cpp, after smh_render.inc and smh_labels.inc.
#include "smh_font5x7_ascii.h"

extern "C" SMHV_API int smhv_text_font(uint8_t ch, uint8_t rows[7]) {
	static const uint8_t font[SMH_TEXT_FONT_GLYPHS][SMH_TEXT_FONT_ROWS] = SMH_FONT5X7_ASCII_TABLE;
	if (!rows) return fail(SMHV_E_INVALID, "text_font: null rows");
	const int g = smh_text_font_index(ch);
	if (g < 0) return fail(SMHV_E_INVALID, "text_font: the font has no glyph for byte 0x%02x", ch);
	memcpy(rows, font[g], SMH_TEXT_FONT_ROWS);
	return SMHV_OK;
}

// debug.rs:388-403: the string the debugger prints, {:?} of a [bool; 3] as Rust writes it
extern "C" SMHV_API int smhv_probe_text(const smhv_probe *p, char *out, size_t cap) {
	if (!p || !out) return fail(SMHV_E_INVALID, "probe_text: null argument");
	char buf[SMH_DBG_TEXT + 56];
	const char *tf[2] = {"false", "true"};
	const uint32_t t = p->team_bits;
	const int n = snprintf(buf, sizeof buf,
	                       "RGB [%u, %u, %u]\nHSV [%u, %u, %u]\nLuma8 %u\nOCRPixelSimilarity %u\nOCRBrightness %u\nAlphaMarker [%s, %s, %s]\n"
	                       "BravoMarker [%s, %s, %s]\nCharlieMarker [%s, %s, %s]",
	                       p->rgb[0], p->rgb[1], p->rgb[2], p->h, p->s, p->v, p->luma, p->mono, p->brightness, tf[t & 1u], tf[(t >> 1) & 1u], tf[(t >> 2) & 1u],
	                       tf[(t >> 3) & 1u], tf[(t >> 4) & 1u], tf[(t >> 5) & 1u], tf[(t >> 6) & 1u], tf[(t >> 7) & 1u], tf[(t >> 8) & 1u]);
	if (n < 0 || (size_t)n + 1u > cap) return fail(SMHV_E_INVALID, "probe_text: %d bytes and the NUL do not fit %zu", n, cap);
	memcpy(out, buf, (size_t)n + 1u);
	return SMHV_OK;
}

// what a call can get wrong in its debug options without the device being asked
static int check_debug_options(const smhv_debug_options *d, const char *what) {
	if (!d) return fail(SMHV_E_INVALID, "%s: null debug options", what);
	if (d->size != sizeof(smhv_debug_options)) return fail(SMHV_E_INVALID, "%s: smhv_debug_options.size %u != %zu", what, d->size, sizeof(smhv_debug_options));
	if (d->flags & ~(SMHV_DEBUG_DRAW_PROBES | SMHV_DEBUG_MINIMAP_CAPTION)) return fail(SMHV_E_INVALID, "%s: unknown debug flags 0x%x", what, d->flags);
	if (d->scale > 4u) return fail(SMHV_E_INVALID, "%s: text scale %u (1 .. 4, 0 = 2)", what, d->scale);
	if (d->n_runs > SMHV_TEXT_MAX_RUNS) return fail(SMHV_E_INVALID, "%s: %u text runs (at most %u)", what, d->n_runs, SMHV_TEXT_MAX_RUNS);
	if (d->n_probes > SMHV_MAX_PROBES) return fail(SMHV_E_INVALID, "%s: %u probes (at most %u)", what, d->n_probes, SMHV_MAX_PROBES);
	if (d->n_runs && !d->runs) return fail(SMHV_E_INVALID, "%s: %u text runs and a null pointer", what, d->n_runs);
	if (d->n_probes && !d->probes) return fail(SMHV_E_INVALID, "%s: %u probes and a null pointer", what, d->n_probes);
	for (uint32_t i = 0; i < d->n_runs; ++i) {
		const smhv_text_run &t = d->runs[i];
		if (t.rgba[3] != 255u) return fail(SMHV_E_INVALID, "%s: text run %u has alpha %u (255 only)", what, i, t.rgba[3]);
		if (t.flags & ~SMHV_TEXT_MAP_COORDS) return fail(SMHV_E_INVALID, "%s: text run %u has unknown flags 0x%x", what, i, t.flags);
		if (t.n > SMHV_TEXT_MAX_BYTES) return fail(SMHV_E_INVALID, "%s: text run %u has %u bytes (at most %u)", what, i, t.n, SMHV_TEXT_MAX_BYTES);
		uint32_t lines = 1u;
		for (uint32_t k = 0; k < t.n; ++k) {
			if (t.text[k] == '\n') ++lines;
			else if (smh_text_font_index(t.text[k]) < 0) return fail(SMHV_E_INVALID, "%s: text run %u: the font has no glyph for byte 0x%02x", what, i, t.text[k]);
		}
		if (lines > SMHV_TEXT_MAX_LINES) return fail(SMHV_E_INVALID, "%s: text run %u has %u lines (at most %u)", what, i, lines, SMHV_TEXT_MAX_LINES);
	}
	return SMHV_OK;
}

#define SMH_DBG_STAGE_BYTES (sizeof(smhv_text_run) * SMHV_TEXT_MAX_RUNS + sizeof(smhv_probe_point) * SMHV_MAX_PROBES)
// the points alone
static const smhv_debug_options *probe_options(smhv_debug_options *d, const smhv_probe_point *points, uint32_t n_points) {
	memset(d, 0, sizeof *d);
	d->size = sizeof *d;
	d->n_probes = n_points; d->probes = points;
	return d;
}

// The batch's probe slab and staging (first call) and, for a call that draws, the item lists and the string pool (first such call);
// the runs and the points through pinned staging onto `s` (waits, host, for the previous call's copy to have read the staging; `s`
// waits for the previous call's kernels, which read the device copy), and the launch arguments but for the frames' own pointers.
static int debug_prepare(smhv_batch *b, const smhv_render_options *ropt, const smhv_debug_options *d, bool draw, hipStream_t s, DebugRun *r) {
	const size_t frames = (size_t)b->max_frames;
	if (!b->d_probes) {                                            // the event first: a failure of the slabs takes it back with them
		hipError_t e = hipEventCreateWithFlags(&b->ev_dbg, hipEventDisableTiming);
		if (e != hipSuccess) { b->ev_dbg = nullptr; return fail(SMHV_E_HIP, "probe slab (%u frames): %s", b->max_frames, hipGetErrorString(e)); }
		int rc = first_use_slabs(b, "probe slab (%u frames)", {{(void **)&b->d_probes, sizeof(smhv_probe) * SMHV_MAX_PROBES * frames, 0},
		                                                       {(void **)&b->d_dbg_stage, SMH_DBG_STAGE_BYTES, SLAB_NO_FILL},
		                                                       {(void **)&b->h_dbg_stage, SMH_DBG_STAGE_BYTES, SLAB_PINNED_HOST}});
		if (rc) { (void)hipEventDestroy(b->ev_dbg); b->ev_dbg = nullptr; return rc; }
	} else
		HIPCHK(hipStreamWaitEvent(s, b->ev_dbg, 0));
	if (draw) {
		int rc = first_use_slabs(b, "debug item lists (%u frames)", {{(void **)&b->d_dbg_items, sizeof(DebugItem) * SMH_DBG_ITEMS * frames, 0},
		                                                             {(void **)&b->d_dbg_pool, (size_t)SMHV_MAX_PROBES * SMH_DBG_TEXT * frames, SLAB_NO_FILL}});
		if (rc) return rc;
	}
	const size_t run_bytes = sizeof(smhv_text_run) * (size_t)d->n_runs, point_bytes = sizeof(smhv_probe_point) * (size_t)d->n_probes;
	const size_t point_off = sizeof(smhv_text_run) * SMHV_TEXT_MAX_RUNS;
	if (run_bytes || point_bytes) {
		if (!b->ev_dbg_stage) HIPCHK(hipEventCreateWithFlags(&b->ev_dbg_stage, hipEventDisableTiming));
		else HIPCHK(wait_event(b->ev_dbg_stage));
		if (run_bytes) {
			memcpy(b->h_dbg_stage, d->runs, run_bytes);
			HIPCHK(hipMemcpyAsync(b->d_dbg_stage, b->h_dbg_stage, run_bytes, hipMemcpyHostToDevice, s));
		}
		if (point_bytes) {
			memcpy(b->h_dbg_stage + point_off, d->probes, point_bytes);
			HIPCHK(hipMemcpyAsync(b->d_dbg_stage + point_off, b->h_dbg_stage + point_off, point_bytes, hipMemcpyHostToDevice, s));
		}
		HIPCHK(hipEventRecord(b->ev_dbg_stage, s));
	}
	memset(r, 0, sizeof *r);
	r->runs = (const smhv_text_run *)b->d_dbg_stage;
	r->points = (const smhv_probe_point *)(b->d_dbg_stage + point_off);
	r->n_runs = d->n_runs; r->n_points = d->n_probes;
	r->flags = d->flags;
	r->scale = d->scale ? d->scale : 2u;
	r->out_w = ropt->out_w; r->out_h = ropt->out_h;
	r->img_stride = (uint64_t)ropt->out_w * ropt->out_h * 4u;
	r->sw = view_scale(ropt->viewport_scale[0]);
	r->sh = view_scale(ropt->viewport_scale[1]);
	r->tx = ropt->viewport_top_left[0]; r->ty = ropt->viewport_top_left[1];
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_batch_probe(smhv_batch *b, uint32_t first, uint32_t n, const smhv_render_options *ropt, const smhv_probe_point *points,
                                         uint32_t n_points, void *stream) {
	if (!b) return fail(SMHV_E_INVALID, "batch_probe: null batch");
	CTX_OPEN(b->ctx);
	if (!ropt) return fail(SMHV_E_INVALID, "batch_probe: null options");
	if (ropt->size != sizeof(smhv_render_options)) return fail(SMHV_E_INVALID, "batch_probe: smhv_render_options.size %u != %zu", ropt->size, sizeof(smhv_render_options));
	if (n_points > SMHV_MAX_PROBES) return fail(SMHV_E_INVALID, "batch_probe: %u points (at most %u)", n_points, SMHV_MAX_PROBES);
	if (n_points && !points) return fail(SMHV_E_INVALID, "batch_probe: %u points and a null pointer", n_points);
	int rc = check_frames(b, first, n, "batch_probe");
	if (rc) return rc;
	if (!b->ui_written) return fail(SMHV_E_STATE, "batch_probe: no run of this batch has produced a ui_map (SMHV_STAGE_UI_MAP)");
	HIPCHK(hipSetDevice(b->ctx->device));
	hipStream_t s = (hipStream_t)stream;
	smhv_debug_options d;
	DebugRun r;
	rc = debug_prepare(b, ropt, probe_options(&d, points, n_points), false, s, &r);
	if (rc) return rc;
	rc = batch_materialize_ui(b, s);                              // the RGBA slab is made when it is read (smh_runtime.cpp)
	if (rc) return rc;
	r.ui = b->d_ui + (size_t)first * b->g.ui_stride;
	r.aux = b->d_aux + first;
	r.res = b->d_results + first;
	r.probes = b->d_probes + (size_t)first * SMHV_MAX_PROBES;
	HIPCHK(launch_debug_text(b->g, r, n, s));
	HIPCHK(hipEventRecord(b->ev_dbg, s));
	b->probed = true;
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_batch_read_probes(smhv_batch *b, uint32_t first, uint32_t n, smhv_probe *out) {
	return batch_read_slab(b, b && b->probed ? b->d_probes : nullptr, sizeof(smhv_probe) * SMHV_MAX_PROBES, first, n, out, "batch_read_probes", "this batch has not probed");
}

extern "C" SMHV_API int smhv_batch_probes_ptr(smhv_batch *b, void **d_probes) {
	return batch_slab_ptr(b, b && b->probed ? b->d_probes : nullptr, d_probes, "batch_probes_ptr", "this batch has not probed");
}

extern "C" SMHV_API int smhv_batch_render_debug(smhv_batch *b, uint32_t first, uint32_t n, const smhv_render_options *ropt, const smhv_debug_options *dopt,
                                                void *stream) {
	if (!b) return fail(SMHV_E_INVALID, "batch_render_debug: null batch");
	CTX_OPEN(b->ctx);
	smhv_render_options o{};                                       // this pass draws no overlay and needs no heightmap for that flag
	const bool sized = ropt && ropt->size == sizeof o;
	if (sized) { o = *ropt; o.flags &= ~SMHV_RENDER_HEIGHTMAP; }
	int rc = check_render_options(sized ? &o : ropt, nullptr, "batch_render_debug");
	if (rc) return rc;
	rc = check_debug_options(dopt, "batch_render_debug");
	if (rc) return rc;
	rc = check_frames(b, first, n, "batch_render_debug");
	if (rc) return rc;
	if (!b->d_render) return fail(SMHV_E_STATE, "batch_render_debug: this batch has not rendered");
	rc = check_window_is_last_render(b, ropt, "batch_render_debug");
	if (rc) return rc;
	HIPCHK(hipSetDevice(b->ctx->device));
	hipStream_t s = (hipStream_t)stream;
	HIPCHK(hipStreamWaitEvent(s, b->ev_render, 0));               // behind the render and the labels that drew the images, whatever stream they took
	DebugRun r;
	rc = debug_prepare(b, ropt, dopt, true, s, &r);
	if (rc) return rc;
	rc = batch_materialize_ui(b, s);                              // the RGBA slab is made when it is read (smh_runtime.cpp)
	if (rc) return rc;
	r.ui = b->d_ui + (size_t)first * b->g.ui_stride;
	r.aux = b->d_aux + first;
	r.res = b->d_results + first;
	r.probes = b->d_probes + (size_t)first * SMHV_MAX_PROBES;
	r.items = b->d_dbg_items + (size_t)first * SMH_DBG_ITEMS;
	r.pool = b->d_dbg_pool + (size_t)first * (SMHV_MAX_PROBES * SMH_DBG_TEXT);
	r.img = b->d_render + (size_t)first * r.img_stride;
	HIPCHK(launch_debug_text(b->g, r, n, s));
	HIPCHK(hipEventRecord(b->ev_dbg, s));
	HIPCHK(hipEventRecord(b->ev_render, s));                      // (the slab's next owner waits for this pass too)
	b->probed = true;
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_render_map_debug(smhv_ctx *c, const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_render_layers *layers,
                                              const smhv_line *lines, uint32_t n_lines, const smhv_label_options *lopt, const smhv_debug_options *dopt,
                                              uint8_t *rgba, smhv_label_result *labels, smhv_probe *probes) {
	const int rc = check_debug_options(dopt, "render_map_debug");
	if (rc) return rc;
	return render_map_per_call(c, hm, ropt, layers, lines, n_lines, lopt, dopt, rgba, labels, probes, PER_CALL_TEXT, "render_map_debug");
}
