// smh_render.inc -- the map view and its layers: public entry points (smh_vision_hip.h, "map view" and "map view: layers"; device
// code in smh_render.hip, k_render_map and k_render_map_layers), and the one per-call path of every form of smhv_render_map.
// Included at the end of smh_runtime.cpp, in front of the text passes that draw over its images.
#define SMH_RENDER_MAX_DIM 16384u
static const float SMH_MAX_ZOOM = 4.0f;          // src/ui/map.rs:128-129
static const uint32_t SMH_ZOOM_LEVELS = 10u;

// MapViewport::calc (src/ui/map.rs:21-77), restated in f32.  This translation unit is compiled with -ffp-contract=off: every
// operation below is one f32 operation.
extern "C" SMHV_API int smhv_map_viewport_calc(float region_w, float region_h, float map_w, float map_h, uint32_t zoom, const float zoom_pos[2],
                                               const float pan_pos[2], smhv_render_options *opt) {
	if (!opt) return fail(SMHV_E_INVALID, "map_viewport_calc: null options");
	const float map_ar = map_w / map_h, win_ar = region_w / region_h;
	float size[2];
	if (win_ar > map_ar) { size[0] = region_h * map_ar; size[1] = region_h; }
	else { const float inv_ar = map_h / map_w; size[0] = region_w; size[1] = region_w * inv_ar; }
	float tl[2] = {(region_w - size[0]) / 2.0f, (region_h - size[1]) / 2.0f};
	if (zoom != 0u) {
		const float zx = zoom_pos ? zoom_pos[0] : 0.0f, zy = zoom_pos ? zoom_pos[1] : 0.0f;
		const float px = pan_pos ? pan_pos[0] : 0.0f, py = pan_pos ? pan_pos[1] : 0.0f;
		const float level = (float)(zoom > 255u ? 255u : zoom);                     // (the app's level is a u8)
		float amount = fminf(level / (float)SMH_ZOOM_LEVELS, 1.0f) * SMH_MAX_ZOOM;
		tl[0] -= zx * size[0] * amount;
		tl[1] -= zy * size[1] * amount;
		tl[0] += px * (size[0] / map_w);
		tl[1] += py * (size[1] / map_h);
		amount += 1.0f;
		size[0] *= amount;
		size[1] *= amount;
	}
	opt->quad[0] = tl[0]; opt->quad[1] = tl[1];
	opt->quad[2] = tl[0] + size[0]; opt->quad[3] = tl[1] + size[1];
	opt->viewport_scale[0] = size[0] / map_w; opt->viewport_scale[1] = size[1] / map_h;
	opt->viewport_top_left[0] = tl[0]; opt->viewport_top_left[1] = tl[1];
	return SMHV_OK;
}

static int check_render_options(const smhv_render_options *opt, const smhv_heightmap *hm, const char *what) {
	if (!opt) return fail(SMHV_E_INVALID, "%s: null options", what);
	if (opt->size != sizeof(smhv_render_options)) return fail(SMHV_E_INVALID, "%s: smhv_render_options.size %u != %zu", what, opt->size, sizeof(smhv_render_options));
	if (opt->flags & ~(SMHV_RENDER_HEIGHTMAP | SMHV_RENDER_MARKERS | SMHV_RENDER_BOUNDS_OFFSET)) return fail(SMHV_E_INVALID, "%s: unknown render flags 0x%x", what, opt->flags);
	if (opt->out_w == 0u || opt->out_h == 0u || opt->out_w > SMH_RENDER_MAX_DIM || opt->out_h > SMH_RENDER_MAX_DIM)
		return fail(SMHV_E_INVALID, "%s: window %u x %u (1 .. %u each)", what, opt->out_w, opt->out_h, SMH_RENDER_MAX_DIM);
	if ((opt->flags & SMHV_RENDER_HEIGHTMAP) && !hm) return fail(SMHV_E_INVALID, "%s: SMHV_RENDER_HEIGHTMAP needs a heightmap", what);
	for (int i = 0; i < 4; ++i)
		if (!std::isfinite(opt->quad[i])) return fail(SMHV_E_INVALID, "%s: quad[%d] is not finite", what, i);
	return SMHV_OK;
}

// The launch arguments of a render of frames [first, first + n) of `b` with the records at `res` (frame `first`'s), after
// everything that can fail without the device has been checked; grows the slab.  Nothing is enqueued before this returns SMHV_OK.
static int render_prepare(smhv_batch *b, uint32_t first, uint32_t n, const smhv_frame_result *res, const smhv_heightmap *hm, const smhv_render_options *opt,
                          RenderRun *r) {
	const Geom &g = b->g;
	const bool use_hm = (opt->flags & SMHV_RENDER_HEIGHTMAP) != 0u;
	const uint32_t *lut = nullptr;
	if (use_hm) {
		int rc = check_hm_device(hm, b->ctx->device, "render", "batch");
		if (rc) return rc;
		rc = hm_lut(hm, &lut);
		if (rc) return rc;
	}
	const uint64_t stride = (uint64_t)opt->out_w * opt->out_h * 4u;
	const uint64_t need = stride * (uint64_t)b->max_frames;       // the whole batch: rendering it in parts keeps the earlier parts
	if (!b->ev_render) HIPCHK(hipEventCreateWithFlags(&b->ev_render, hipEventDisableTiming));
	if (b->render_cap < need) {
		if (b->d_render) {
			HIPCHK(wait_event(b->ev_render));                    // the previous render has left the old slab
			(void)hipFree(b->d_render);
			b->d_render = nullptr; b->render_cap = 0;
		}
		hipError_t e = hipMalloc((void **)&b->d_render, (size_t)need);
		if (e != hipSuccess) { b->d_render = nullptr; return fail(SMHV_E_HIP, "render slab (%llu bytes): %s", (unsigned long long)need, hipGetErrorString(e)); }
		b->render_cap = (size_t)need;
	}
	b->render_w = opt->out_w; b->render_h = opt->out_h;
	memset(r, 0, sizeof *r);
	r->ui = b->d_ui + (size_t)first * g.ui_stride;
	r->out = b->d_render + (size_t)first * stride;
	r->aux = b->d_aux + first;
	r->res = res;
	r->out_stride = stride;
	if (use_hm) {
		r->hm = hm->d; r->lut = lut; r->hm_w = hm->w; r->hm_h = hm->h;
		r->lut16 = (const uint16_t *)(lut + SMH_HM_LUT_ENTRIES + 4u);
		r->b0x = (float)hm->bounds[0]; r->b0y = (float)hm->bounds[1];
	}
	r->flags = opt->flags;
	r->out_w = opt->out_w; r->out_h = opt->out_h;
	r->ql = opt->quad[0]; r->qt = opt->quad[1]; r->qr = opt->quad[2]; r->qb = opt->quad[3];
	r->sw = view_scale(opt->viewport_scale[0]);
	r->sh = view_scale(opt->viewport_scale[1]);
	r->tx = opt->viewport_top_left[0]; r->ty = opt->viewport_top_left[1];
	memcpy(&r->bg, opt->background, 4);
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_batch_render_ptr(smhv_batch *b, void **d_images, uint64_t *stride) {
	if (!b || !d_images) return fail(SMHV_E_INVALID, "batch_render_ptr: null argument");
	if (!b->d_render) return fail(SMHV_E_STATE, "batch_render_ptr: this batch has not rendered");
	*d_images = b->d_render;
	if (stride) *stride = (uint64_t)b->render_w * b->render_h * 4u;
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_batch_render_size(smhv_batch *b, uint32_t *out_w, uint32_t *out_h) {
	if (!b || !out_w || !out_h) return fail(SMHV_E_INVALID, "batch_render_size: null argument");
	if (!b->d_render) return fail(SMHV_E_STATE, "batch_render_size: this batch has not rendered");
	*out_w = b->render_w; *out_h = b->render_h;
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_batch_read_render(smhv_batch *b, uint32_t frame, uint8_t *rgba) {
	if (!b || !rgba || frame >= b->max_frames) return fail(SMHV_E_INVALID, "batch_read_render: bad arguments");
	if (!b->d_render) return fail(SMHV_E_STATE, "batch_read_render: this batch has not rendered");
	const size_t stride = (size_t)b->render_w * b->render_h * 4u;
	if (((size_t)frame + 1u) * stride > b->render_cap) return fail(SMHV_E_INVALID, "batch_read_render: frame %u lies beyond the render slab", frame);
	HIPCHK(hipSetDevice(b->ctx->device));
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpy(rgba, b->d_render + (size_t)frame * stride, stride, hipMemcpyDeviceToHost));
	return SMHV_OK;
}

// ---- the map view with layers (smh_vision_hip.h, "map view: layers"; k_render_map_layers) ----
static int check_render_layers(const smhv_render_layers *ly, const char *what) {
	if (!ly) return fail(SMHV_E_INVALID, "%s: null layers", what);
	if (ly->size != sizeof(smhv_render_layers)) return fail(SMHV_E_INVALID, "%s: smhv_render_layers.size %u != %zu", what, ly->size, sizeof(smhv_render_layers));
	if (ly->flags & ~SMHV_LAYER_MINIMAP_BOUNDS) return fail(SMHV_E_INVALID, "%s: unknown layer flags 0x%x", what, ly->flags);
	if (ly->map_source > (uint32_t)SMHV_VIEW_CROPPED_BRQ) return fail(SMHV_E_INVALID, "%s: unknown map source %u", what, ly->map_source);
	if (ly->n_prims > SMHV_RENDER_MAX_PRIMS) return fail(SMHV_E_INVALID, "%s: %u prims (at most %u)", what, ly->n_prims, SMHV_RENDER_MAX_PRIMS);
	if (ly->n_prims && !ly->prims) return fail(SMHV_E_INVALID, "%s: %u prims and a null pointer", what, ly->n_prims);
	for (uint32_t i = 0; i < ly->n_prims; ++i) {
		const smhv_render_prim &p = ly->prims[i];
		if ((p.kind & ~(0xFFu | SMHV_PRIM_FOREGROUND | SMHV_PRIM_SHIFT1)) || (p.kind & 0xFFu) > SMHV_PRIM_RECT)
			return fail(SMHV_E_INVALID, "%s: prim %u has the unknown kind 0x%x", what, i, p.kind);
		if (p.rgba[3] != 255u) return fail(SMHV_E_INVALID, "%s: prim %u has alpha %u (255 only)", what, i, p.rgba[3]);
	}
	return SMHV_OK;
}

// The prims of a call on their way to the device: the list is split in paint order -- those below the marker lines, then the
// foreground ones, each part in list order -- into the batch's pinned staging and copied on `s`.  Waits (host) for the previous
// call's copy to have read the staging.  Fills y->prims, n_below, n_fg.
static int render_upload_prims(smhv_batch *b, const smhv_render_layers *ly, RenderLayersRun *y, hipStream_t s) {
	if (ly->n_prims == 0u) return SMHV_OK;
	const size_t cap = sizeof(smhv_render_prim) * (size_t)SMHV_RENDER_MAX_PRIMS;
	if (!b->h_prims) HIPCHK(hipHostMalloc((void **)&b->h_prims, cap));
	if (!b->d_prims) HIPCHK(hipMalloc((void **)&b->d_prims, cap));
	if (!b->ev_prims) HIPCHK(hipEventCreateWithFlags(&b->ev_prims, hipEventDisableTiming));
	else HIPCHK(wait_event(b->ev_prims));
	uint32_t k = 0;
	for (uint32_t pass = 0; pass < 2u; ++pass) {
		for (uint32_t i = 0; i < ly->n_prims; ++i)
			if (((ly->prims[i].kind & SMHV_PRIM_FOREGROUND) != 0u) == (pass == 1u)) b->h_prims[k++] = ly->prims[i];
		if (pass == 0u) y->n_below = k;
	}
	y->n_fg = k - y->n_below;
	y->prims = b->d_prims;
	HIPCHK(hipMemcpyAsync(b->d_prims, b->h_prims, sizeof(smhv_render_prim) * (size_t)k, hipMemcpyHostToDevice, s));
	HIPCHK(hipEventRecord(b->ev_prims, s));
	return SMHV_OK;
}

// The map of a batch's layers call: the ui_map, or one of the images the batch's runs left behind, from frame `first` on.  Refuses a
// source no run has produced; enqueues nothing.
static int batch_render_source(smhv_batch *b, uint32_t first, const smhv_render_layers *layers, RenderLayersRun *y) {
	const Geom &g = b->g;
	y->flags = layers->flags;
	y->src_mode = SMH_RND_SRC_UI; y->src_w = g.rw; y->src_h = g.rh;
	switch ((int)layers->map_source) {
	case SMHV_VIEW_NONE: break;
	case SMHV_VIEW_OCR_INPUT:
	case SMHV_VIEW_FIND_SCALES_INPUT: {
		const bool ocr = layers->map_source == (uint32_t)SMHV_VIEW_OCR_INPUT;
		if (!(ocr ? b->ocr_written : b->scales_written))
			return fail(SMHV_E_STATE, "batch_render_layers: no run of this batch has produced the %s image", ocr ? "OCR input (SMHV_STAGE_OCR)" : "scales input (SMHV_STAGE_SCALES with anchors)");
		y->src_mode = SMH_RND_SRC_GRAY; y->src = (ocr ? b->d_ocr : b->d_scales) + (size_t)first * g.ocr_stride;
		y->src_pitch = g.ocr_pitch; y->src_stride = g.ocr_stride; y->src_xoff = g.q_xoff; y->src_w = g.qw; y->src_h = g.qh;
		break;
	}
	case SMHV_VIEW_LSD_INPUT:
		if (!b->mask_written) return fail(SMHV_E_STATE, "batch_render_layers: no run of this batch has produced the marker mask (SMHV_STAGE_MARKERS)");
		y->src_mode = SMH_RND_SRC_GRAY; y->src = b->d_mask + (size_t)first * g.mask_stride;
		y->src_pitch = g.mask_pitch; y->src_stride = g.mask_stride; y->src_xoff = g.m_xoff;
		break;
	default:                                                   // SMHV_VIEW_LSD_PREPROCESS, SMHV_VIEW_CROPPED_BRQ: the colour ui_map
		if (b->ui_gray) return fail(SMHV_E_STATE, "batch_render_layers: the batch's ui_map is grayscale, map source %u needs the colour one", layers->map_source);
		if (layers->map_source == (uint32_t)SMHV_VIEW_CROPPED_BRQ) {
			y->src_mode = SMH_RND_SRC_CROPPED; y->src_w = g.rw / 2u; y->src_h = g.rh / 2u;
			if (y->src_w == 0u || y->src_h == 0u) return fail(SMHV_E_STATE, "batch_render_layers: the map has no bottom right quarter");
		} else y->src_mode = SMH_RND_SRC_PREPROCESS;
		break;
	}
	return SMHV_OK;
}

// smhv_batch_render (with_layers false: k_render_map) and smhv_batch_render_layers (k_render_map_layers), `what` in the messages
static int batch_render(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *opt, bool with_layers,
                        const smhv_render_layers *layers, hipStream_t s, const char *what) {
	if (!b) return fail(SMHV_E_INVALID, "%s: null batch", what);
	CTX_OPEN(b->ctx);
	int rc = check_render_options(opt, hm, what);
	if (rc) return rc;
	if (with_layers) {
		rc = check_render_layers(layers, what);
		if (rc) return rc;
	}
	rc = check_frames(b, first, n, what);
	if (rc) return rc;
	if (!b->ui_written) return fail(SMHV_E_STATE, "%s: no run of this batch has produced a ui_map (SMHV_STAGE_UI_MAP)", what);
	const Geom &g = b->g;
	RenderLayersRun y{};
	if (with_layers) {
		rc = batch_render_source(b, first, layers, &y);
		if (rc) return rc;
	}
	HIPCHK(hipSetDevice(b->ctx->device));
	const bool use_hm = (opt->flags & SMHV_RENDER_HEIGHTMAP) != 0u;
	RenderRun r;
	rc = render_prepare(b, first, n, b->d_results + first, use_hm ? hm : nullptr, opt, &r);
	if (rc) return rc;
	if (with_layers && layers->map_source == (uint32_t)SMHV_VIEW_LSD_INPUT) {  // the mask as bytes is made when it is read
		rc = batch_materialize_mask(b, s);
		if (rc) return rc;
	}
	rc = batch_materialize_ui(b, s);                           // ... and so is the RGBA ui slab
	if (rc) return rc;
	if (with_layers) {
		rc = render_upload_prims(b, layers, &y, s);
		if (rc) return rc;
	}
	hm_rebind(&b->render_hm, use_hm ? hm : nullptr);           // the batch's reference of the heightmap its enqueued render reads
	rc = for_each_launch(n, [&](uint32_t done, uint32_t k) -> int {
		RenderRun part = r;
		part.ui += (size_t)done * g.ui_stride; part.out += (size_t)done * r.out_stride; part.aux += done; part.res += done;
		RenderLayersRun yp = y;
		if (yp.src) yp.src += (size_t)done * y.src_stride;
		HIPCHK(with_layers ? launch_render_map_layers(g, part, yp, k, s) : launch_render_map(g, part, k, s));
		return SMHV_OK;
	});
	if (rc) return rc;
	HIPCHK(hipEventRecord(b->ev_render, s));
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_batch_render(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *opt, void *stream) {
	return batch_render(b, first, n, hm, opt, false, nullptr, (hipStream_t)stream, "batch_render");
}

extern "C" SMHV_API int smhv_batch_render_layers(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *opt,
                                                 const smhv_render_layers *layers, void *stream) {
	return batch_render(b, first, n, hm, opt, true, layers, (hipStream_t)stream, "batch_render_layers");
}

// ---- the per-call map view: smhv_render_map, _layers, _labeled (smh_labels.inc) and _debug (smh_debugtext.inc) ----
// the text passes' side of it, defined in the files included after this one
static int check_label_options(const smhv_label_options *lo, const char *what);
static int labels_prepare(smhv_batch *b, const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_label_options *lo, hipStream_t s, LabelRun *r);
static int debug_prepare(smhv_batch *b, const smhv_render_options *ropt, const smhv_debug_options *dopt, bool draw, hipStream_t s, DebugRun *r);

// what an entry point asks of its arguments beyond the plain smhv_render_map's
enum : uint32_t {
	PER_CALL_LAYERS = 1u,                                      // `layers` may not be NULL
	PER_CALL_TEXT = 2u,                                        // label options unless `dopt` is given; a heightmap of another device is refused even when no overlay is drawn
};

// The current frame: frame 0 of the single-frame batch's ui slab (crop_to_map's pass), the rectangle of crop_to_map's walk (the
// minimap's own record slot, 3), the caller's lines through the context's pinned staging; drawn into that batch's render slab on
// the context's stream -- by k_render_map, or with `layers` by k_render_map_layers --, then the labels (`lopt`) and the debug pass
// (`dopt`, checked by its caller) over the image, which is copied out once, after them.  fire_mu from render_prepare to the last
// copy, mu around the read-back's staging.
static int render_map_per_call(smhv_ctx *c, const smhv_heightmap *hm, const smhv_render_options *opt, const smhv_render_layers *layers, const smhv_line *lines,
                               uint32_t n_lines, const smhv_label_options *lopt, const smhv_debug_options *dopt, uint8_t *rgba, smhv_label_result *labels,
                               smhv_probe *probes, uint32_t asks, const char *what) {
	int rc = require_open(c, what);
	if (rc) return rc;
	CTX_OPEN(c);
	if (!rgba || (n_lines && !lines)) return fail(SMHV_E_INVALID, "%s: null argument", what);
	if (n_lines > SMHV_RENDER_MAX_LINES) return fail(SMHV_E_INVALID, "%s: %u lines (at most %u)", what, n_lines, SMHV_RENDER_MAX_LINES);
	rc = check_render_options(opt, hm, what);
	if (rc) return rc;
	if (layers || (asks & PER_CALL_LAYERS)) {
		rc = check_render_layers(layers, what);
		if (rc) return rc;
	}
	if (asks & PER_CALL_TEXT) {
		if (lopt || !dopt) {
			rc = check_label_options(lopt, what);
			if (rc) return rc;
		}
		if (lopt && (lopt->flags & SMHV_LABEL_DETECTED) && n_lines > SMHV_MAX_LINES)
			return fail(SMHV_E_INVALID, "%s: %u detected lines to label (at most %u)", what, n_lines, (unsigned)SMHV_MAX_LINES);
		rc = check_hm_device(hm, c->device, what, "context");
		if (rc) return rc;
	}
	HIPCHK(hipSetDevice(c->device));
	smhv_batch *b = c->fb;
	const Geom &g = b->g;
	const bool use_hm = (opt->flags & SMHV_RENDER_HEIGHTMAP) != 0u;
	std::lock_guard<std::mutex> lk(c->fire_mu);
	RenderRun r;
	rc = render_prepare(b, 0, 1, b->d_results + 3, use_hm ? hm : nullptr, opt, &r);
	if (rc) return rc;
	RenderLayersRun y{};
	uint8_t *d_view = nullptr;
	if (layers) {
		y.flags = layers->flags;
		y.src_mode = SMH_RND_SRC_UI; y.src_w = g.rw; y.src_h = g.rh;
		if (layers->map_source != (uint32_t)SMHV_VIEW_NONE) {
			// U = smhv_get_debug_view's image of this moment: drawn by its kernel into device memory and sampled there
			debug_view_size(g, (int)layers->map_source, &y.src_w, &y.src_h);
			HIPCHK(hipMalloc((void **)&d_view, (size_t)y.src_w * y.src_h * 4u));
			hipError_t e = ctx_debug_view(c, (int)layers->map_source, d_view);
			if (e != hipSuccess) { (void)hipFree(d_view); return fail(SMHV_E_HIP, "%s: debug view: %s", what, hipGetErrorString(e)); }
			y.src_mode = SMH_RND_SRC_RGBA; y.src = d_view; y.src_pitch = (uint64_t)y.src_w * 4u;
		}
	}
	const auto run = [&]() -> int {
		int rc2 = ctx_stage_reserve(c, sizeof(smhv_line) * (size_t)SMHV_RENDER_MAX_LINES);
		if (rc2) return rc2;
		const bool label_lines = lopt && n_lines && (lopt->flags & SMHV_LABEL_DETECTED);
		if (n_lines && ((opt->flags & SMHV_RENDER_MARKERS) || label_lines)) {
			memcpy(c->h_fire, lines, sizeof(smhv_line) * (size_t)n_lines);
			HIPCHK(hipMemcpyAsync(c->d_fire, c->h_fire, sizeof(smhv_line) * (size_t)n_lines, hipMemcpyHostToDevice, c->s_main));
		}
		if (n_lines && (opt->flags & SMHV_RENDER_MARKERS)) { r.lines = (const smhv_line *)c->d_fire; r.n_lines = n_lines; }
		else r.flags &= ~SMHV_RENDER_MARKERS;                    // (no explicit lines: none are drawn, whatever the spare record holds)
		if (layers) {
			rc2 = render_upload_prims(b, layers, &y, c->s_main);
			if (rc2) return rc2;
			HIPCHK(launch_render_map_layers(g, r, y, 1, c->s_main));
		} else
			HIPCHK(launch_render_map(g, r, 1, c->s_main));
		if (lopt) {
			LabelRun lr;
			rc2 = labels_prepare(b, hm, opt, lopt, c->s_main, &lr);
			if (rc2) return rc2;
			lr.aux = b->d_aux;
			lr.res = b->d_results + 3;
			lr.per_call = 1u;
			lr.lines = label_lines ? (const smhv_line *)c->d_fire : nullptr;
			lr.n_lines = label_lines ? n_lines : 0u;
			lr.has_mpx = lopt->mpx ? 1u : 0u;
			lr.mpx = lopt->mpx ? *lopt->mpx : 0.0;
			lr.out = b->d_labels;
			lr.cull = b->d_label_cull;
			lr.img = b->d_render;
			HIPCHK(launch_labels(lr, 1, c->s_main));
		}
		if (dopt) {
			DebugRun dr;
			rc2 = debug_prepare(b, opt, dopt, true, c->s_main, &dr);
			if (rc2) return rc2;
			rc2 = batch_materialize_ui(b, c->s_main);              // (the single-frame batch's pass writes RGBA: nothing is ever owed)
			if (rc2) return rc2;
			dr.ui = b->d_ui;
			dr.aux = b->d_aux;
			dr.res = b->d_results + 3;
			dr.probes = b->d_probes;
			dr.items = b->d_dbg_items;
			dr.pool = b->d_dbg_pool;
			dr.img = b->d_render;
			HIPCHK(launch_debug_text(g, dr, 1, c->s_main));
			HIPCHK(hipEventRecord(b->ev_dbg, c->s_main));
			b->probed = true;
		}
		HIPCHK(hipEventRecord(b->ev_render, c->s_main));
		std::lock_guard<std::mutex> lk2(c->mu);                  // (staging slot 2: the batch read-back's)
		rc2 = copy_image_d2h(c, 2, rgba, b->d_render, (size_t)r.out_stride / opt->out_h, 0, (size_t)opt->out_w * 4, opt->out_h, c->s_main);
		if (rc2) return rc2;
		if (labels && lopt) HIPCHK(hipMemcpy(labels, b->d_labels, sizeof(smhv_label_result), hipMemcpyDeviceToHost));   // (the stream has run dry)
		if (probes && dopt) HIPCHK(hipMemcpy(probes, b->d_probes, sizeof(smhv_probe) * SMHV_MAX_PROBES, hipMemcpyDeviceToHost));
		return SMHV_OK;
	};
	rc = run();
	if (d_view) {
		if (rc) (void)hipStreamSynchronize(c->s_main);           // (whatever was enqueued has left the view before it goes)
		(void)hipFree(d_view);
	}
	return rc;
}

extern "C" SMHV_API int smhv_render_map(smhv_ctx *c, const smhv_heightmap *hm, const smhv_render_options *opt, const smhv_line *lines, uint32_t n_lines,
                                        uint8_t *rgba) {
	return render_map_per_call(c, hm, opt, nullptr, lines, n_lines, nullptr, nullptr, rgba, nullptr, nullptr, 0u, "render_map");
}

extern "C" SMHV_API int smhv_render_map_layers(smhv_ctx *c, const smhv_heightmap *hm, const smhv_render_options *opt, const smhv_render_layers *layers,
                                               const smhv_line *lines, uint32_t n_lines, uint8_t *rgba) {
	return render_map_per_call(c, hm, opt, layers, lines, n_lines, nullptr, nullptr, rgba, nullptr, nullptr, PER_CALL_LAYERS, "render_map_layers");
}

extern "C" SMHV_API int smhv_debug_render_form(uint32_t form) {
	if (form > 3u) return fail(SMHV_E_INVALID, "render form %u (0 = the rule, 1 = gathers, 2 = LDS staging, 3 = the colour table in LDS)", form);
	render_set_form(form);
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_debug_render_rule(uint32_t map_w, uint32_t map_h, float sw, float sh, uint32_t hm_w, uint32_t hm_h, float *ratio, float *switch_ratio,
                                               uint32_t *lds_texels, uint32_t *form) {
	if (!map_w || !map_h || !hm_w || !hm_h) return fail(SMHV_E_INVALID, "render_rule: zero dimension");
	Geom g{};
	g.rw = map_w; g.rh = map_h;
	RenderRun r{};
	r.sw = view_scale(sw); r.sh = view_scale(sh); r.hm_w = hm_w; r.hm_h = hm_h;
	float ra = 0.0f;
	uint32_t tx = 0;
	const uint32_t f = render_rule(g, r, &tx, &ra);
	if (ratio) *ratio = ra;
	if (switch_ratio) *switch_ratio = render_switch_ratio();
	if (lds_texels) *lds_texels = tx;
	if (form) *form = f;
	return SMHV_OK;
}
