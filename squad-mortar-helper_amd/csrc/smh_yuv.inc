// smh_yuv.inc -- host side of the 4:2:0 video layouts (SMHV_PIXELS_NV12 / _I420; device code in smh_yuv.hip).  Included by
// smh_runtime.cpp in front of the ingest queue, which uses the helpers here.

struct YuvDesc { uint32_t layout, matrix, full, bilinear; };

// SMHV_PIXELS_YUV(...) -> its parts; false for another layout or an unknown bit
static bool yuv_decode(uint32_t pixels, YuvDesc *d) {
	const uint32_t layout = pixels & 0xFFu;
	if ((layout != SMHV_PIXELS_NV12 && layout != SMHV_PIXELS_I420) || (pixels & ~0x7FFu)) return false;
	d->layout = layout; d->matrix = (pixels >> 8) & 1u; d->full = (pixels >> 9) & 1u; d->bilinear = (pixels >> 10) & 1u;
	return true;
}

static YuvCoef yuv_coef(const YuvDesc &d) {
	static const YuvCoef table[2][2] = {{{298, 16, 459, 55, 136, 541}, {298, 16, 409, 100, 208, 516}},      // [full][matrix]
	                                    {{256, 0, 403, 48, 120, 475}, {256, 0, 359, 88, 183, 454}}};
	return table[d.full][d.matrix];
}

static uint64_t yuv_tight_bytes(uint32_t w, uint32_t h) { return (uint64_t)w * h + 2ull * ((w + 1u) / 2u) * ((h + 1u) / 2u); }

// a rectangle of a frame whose samples lie in the frame's own planes
static YuvRect yuv_plane_rect(uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint64_t y_pitch, uint64_t uv_pitch, uint64_t u_off, uint64_t v_off) {
	YuvRect r{};
	r.x0 = x0; r.y0 = y0; r.w = w; r.h = h;
	r.y_off = 0; r.u_off = u_off; r.v_off = v_off;
	r.y_pitch = (uint32_t)y_pitch; r.uv_pitch = (uint32_t)uv_pitch;
	return r;
}

// a tight frame of W x H in `layout` at offset 0
static YuvRect yuv_tight_rect(uint32_t W, uint32_t H, uint32_t layout) {
	const uint64_t cw = (W + 1u) / 2u, ch = (H + 1u) / 2u;
	const uint64_t uvp = layout == SMHV_PIXELS_NV12 ? 2u * cw : cw, u_off = (uint64_t)W * H;
	return yuv_plane_rect(0, 0, W, H, W, uvp, u_off, layout == SMHV_PIXELS_NV12 ? u_off : u_off + uvp * ch);
}

// ---- the packed rows of a rectangle (the ingest queue's region-of-interest upload) -----------------------------------------
// Y: the rectangle's rows from the quad-aligned column y_x0 on; chroma: the rows and columns its pixels lie in plus one of halo
// each way (what bilinear chroma reads), clamped at the frame's edge, from an even column on.  Every pitch and section offset is
// a multiple of 4, so that the kernel's wide loads apply.  The chroma section is sized for I420's two planes; NV12's one
// interleaved plane is no larger.
struct YuvPack {
	uint32_t x0, y0, w, h;
	uint32_t y_x0, y_cols, y_pitch, c_x0, c_cols, c_y0, c_rows;
	uint64_t y_off, c_off, bytes;              // offsets into the pack buffer; bytes of this rectangle's sections
};
static uint32_t align4(uint32_t v) { return (v + 3u) & ~3u; }
static void yuv_pack_geom(uint32_t W, uint32_t H, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint64_t base, YuvPack *p) {
	const uint32_t cw = (W + 1u) / 2u, ch = (H + 1u) / 2u;
	p->x0 = x0; p->y0 = y0; p->w = w; p->h = h;
	p->y_x0 = x0 & ~3u; p->y_cols = x0 + w - p->y_x0; p->y_pitch = align4(p->y_cols);
	p->c_x0 = ((x0 >> 1) ? (x0 >> 1) - 1u : 0u) & ~1u;
	p->c_cols = std::min(((x0 + w - 1u) >> 1) + 1u, cw - 1u) - p->c_x0 + 1u;
	p->c_y0 = (y0 >> 1) ? (y0 >> 1) - 1u : 0u;
	p->c_rows = std::min(((y0 + h - 1u) >> 1) + 1u, ch - 1u) - p->c_y0 + 1u;
	p->y_off = base; p->c_off = base + (uint64_t)p->y_pitch * h;
	p->bytes = (uint64_t)p->y_pitch * h + 2ull * align4(p->c_cols) * p->c_rows;
}
static uint32_t yuv_pack_uv_pitch(const YuvPack &p, uint32_t layout) { return layout == SMHV_PIXELS_NV12 ? align4(2u * p.c_cols) : align4(p.c_cols); }
static YuvRect yuv_pack_rect(const YuvPack &p, uint32_t layout) {
	YuvRect r{};
	r.x0 = p.x0; r.y0 = p.y0; r.w = p.w; r.h = p.h;
	r.y_pitch = p.y_pitch; r.uv_pitch = yuv_pack_uv_pitch(p, layout);
	r.y_off = p.y_off; r.u_off = p.c_off; r.v_off = layout == SMHV_PIXELS_NV12 ? p.c_off : p.c_off + (uint64_t)r.uv_pitch * p.c_rows;
	r.y_x0 = p.y_x0; r.y_y0 = p.y0; r.c_x0 = p.c_x0; r.c_y0 = p.c_y0;
	return r;
}
// copy what rectangle p needs of Y row y / chroma row r of a tight frame into the pack (rows outside the rectangle: nothing)
static void yuv_pack_y_row(const YuvPack &p, uint8_t *pack, uint32_t y, const uint8_t *row) {
	if (y >= p.y0 && y < p.y0 + p.h) memcpy(pack + p.y_off + (size_t)(y - p.y0) * p.y_pitch, row + p.y_x0, p.y_cols);
}
// plane: 0 = U (NV12: the pairs), 1 = V
static void yuv_pack_c_row(const YuvPack &p, uint8_t *pack, uint32_t layout, uint32_t plane, uint32_t r, const uint8_t *row) {
	if (r < p.c_y0 || r >= p.c_y0 + p.c_rows) return;
	const uint32_t pitch = yuv_pack_uv_pitch(p, layout), bpc = layout == SMHV_PIXELS_NV12 ? 2u : 1u;
	memcpy(pack + p.c_off + (size_t)plane * pitch * p.c_rows + (size_t)(r - p.c_y0) * pitch, row + (size_t)p.c_x0 * bpc, (size_t)p.c_cols * bpc);
}

// smhv_yuv_layout as the caller gave it (null, or zero members: tight) -> every member filled in, for n frames of w x h in
// `layout` (SMHV_PIXELS_NV12 / _I420; NV12: v_offset = u_offset).  SMHV_E_INVALID for what the header lists.  Both directions.
static int yuv_resolve_layout(const char *what, uint32_t layout, const smhv_yuv_layout *given, uint32_t n, uint32_t w, uint32_t h, smhv_yuv_layout *out) {
	const uint64_t cw = (w + 1u) / 2u, ch = (h + 1u) / 2u;
	const uint64_t uv_row = layout == SMHV_PIXELS_NV12 ? 2u * cw : cw;
	smhv_yuv_layout L{};
	if (given) L = *given;
	if (!L.y_pitch) L.y_pitch = w;
	if (!L.uv_pitch) L.uv_pitch = uv_row;
	if (L.y_pitch < w || L.uv_pitch < uv_row || L.y_pitch > 0x7FFFFFFFull || L.uv_pitch > 0x7FFFFFFFull)
		return fail(SMHV_E_INVALID, "%s: pitches %llu / %llu for rows of %u / %llu bytes", what, (unsigned long long)L.y_pitch, (unsigned long long)L.uv_pitch, w,
		            (unsigned long long)uv_row);
	if (!L.u_offset) L.u_offset = L.y_pitch * h;
	if (layout == SMHV_PIXELS_NV12) {
		if (L.v_offset && L.v_offset != L.u_offset + 1u) return fail(SMHV_E_INVALID, "%s: NV12 has its V samples at u_offset + 1", what);
		L.v_offset = L.u_offset;
	} else if (!L.v_offset) L.v_offset = L.u_offset + L.uv_pitch * ch;
	// (the last row of a plane ends with its samples, not with its pitch)
	const uint64_t y_end = L.y_pitch * (h - 1u) + w, u_end = L.u_offset + L.uv_pitch * (ch - 1u) + uv_row, v_end = L.v_offset + L.uv_pitch * (ch - 1u) + uv_row;
	const uint64_t frame_end = std::max(y_end, std::max(u_end, v_end));
	if (!L.frame_stride) L.frame_stride = frame_end;
	if (n > 1u && L.frame_stride < frame_end) return fail(SMHV_E_INVALID, "%s: frame_stride %llu, a frame's planes end at %llu", what, (unsigned long long)L.frame_stride,
	                                                      (unsigned long long)frame_end);
	*out = L;
	return SMHV_OK;
}

extern "C" SMHV_API uint64_t smhv_ingest_staging_bytes(uint32_t w, uint32_t h, uint32_t pixels) {
	if (w == 0 || h == 0 || w > 32768u || h > 32768u) { (void)fail(SMHV_E_INVALID, "ingest_staging_bytes: %u x %u (1 .. 32768 each way)", w, h); return 0; }
	YuvDesc d;
	if (yuv_decode(pixels, &d)) return yuv_tight_bytes(w, h);
	switch (pixels) {
	case SMHV_PIXELS_BGRA8: case SMHV_PIXELS_RGBA8: return (uint64_t)w * h * 4u;
	case SMHV_PIXELS_RGB8: return (uint64_t)w * h * 3u;
	case SMHV_PIXELS_LUMA_A8: return (uint64_t)w * h * 2u;
	case SMHV_PIXELS_LUMA8: return (uint64_t)w * h;
	default: (void)fail(SMHV_E_INVALID, "ingest_staging_bytes: unknown pixel layout 0x%x", pixels); return 0;
	}
}

extern "C" SMHV_API int smhv_yuv_to_bgra_device(smhv_ctx *c, const void *d_src, const smhv_yuv_layout *layout, uint32_t n, uint32_t w, uint32_t h, uint32_t pixels,
                                                void *d_bgra, uint64_t out_stride_bytes, uint32_t flags, void *stream) {
	if (!c || !d_src || !d_bgra) return fail(SMHV_E_INVALID, "yuv_to_bgra: null argument");
	if (n == 0 || w == 0 || h == 0 || w > 32768u || h > 32768u) return fail(SMHV_E_INVALID, "yuv_to_bgra: %u frames of %u x %u (1 .. 32768 each way)", n, w, h);
	YuvDesc d;
	if (!yuv_decode(pixels, &d)) return fail(SMHV_E_INVALID, "yuv_to_bgra: pixels 0x%x is not SMHV_PIXELS_YUV(NV12 | I420, matrix, range, chroma)", pixels);
	if (flags & ~SMHV_YUV_ROI_ONLY) return fail(SMHV_E_INVALID, "yuv_to_bgra: unknown flags 0x%x", flags);
	if ((uintptr_t)d_bgra & 3u) return fail(SMHV_E_INVALID, "yuv_to_bgra: the output is not 4-byte aligned");
	const uint64_t out_frame = (uint64_t)w * h * 4u;
	smhv_yuv_layout L;
	int lrc = yuv_resolve_layout("yuv_to_bgra", d.layout, layout, n, w, h, &L);
	if (lrc) return lrc;
	if (!out_stride_bytes) out_stride_bytes = out_frame;
	if (out_stride_bytes < out_frame || (out_stride_bytes & 3u)) return fail(SMHV_E_INVALID, "yuv_to_bgra: out_stride_bytes %llu for frames of %llu bytes (a multiple of 4)",
	                                                                         (unsigned long long)out_stride_bytes, (unsigned long long)out_frame);
	YuvRun run{};
	uint32_t n_rects = 1;
	if (flags & SMHV_YUV_ROI_ONLY) {
		Geom g;
		int rc = compute_geom(w, h, &g);
		if (rc) return rc;
		run.r[0] = yuv_plane_rect(g.rx, g.ry, g.rw, g.rh, L.y_pitch, L.uv_pitch, L.u_offset, L.v_offset);
		run.r[1] = yuv_plane_rect(g.bx, g.by, g.bw, g.bh, L.y_pitch, L.uv_pitch, L.u_offset, L.v_offset);
		n_rects = 2;
	} else run.r[0] = yuv_plane_rect(0, 0, w, h, L.y_pitch, L.uv_pitch, L.u_offset, L.v_offset);
	if (((uint64_t)(h + 1u) / 2u / SMH_YUV_BAND_PAIRS + 2u) * n > 0x7FFFFFFFull) return fail(SMHV_E_INVALID, "yuv_to_bgra: %u frames of %u rows are more than one launch takes", n, h);
	CTX_OPEN(c);
	HIPCHK(hipSetDevice(c->device));
	run.src = (const uint8_t *)d_src; run.dst = (uint8_t *)d_bgra;
	run.src_stride = L.frame_stride; run.dst_stride = out_stride_bytes;
	run.W = w; run.H = h; run.n = n; run.k = yuv_coef(d);
	HIPCHK(launch_yuv_to_bgra(run, n_rects, d.layout, d.bilinear, stream ? (hipStream_t)stream : c->s_main));
	return SMHV_OK;
}
