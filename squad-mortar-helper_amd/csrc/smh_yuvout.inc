// smh_yuvout.inc -- host side of video frames OUT (include/smh_vision_hip.h, "video frames OUT"; device code in smh_yuvout.hip).
// Included by smh_runtime.cpp behind smh_yuv.inc, whose word decoding and layout resolution it shares.

// an output word: SMHV_PIXELS_YUV(layout, matrix, range, 0)
static bool yuv_out_decode(uint32_t pixels, YuvDesc *d) { return yuv_decode(pixels, d) && !d->bilinear; }

static YuvOutCoef yuv_out_coef(const YuvDesc &d) {
	static const YuvOutCoef table[2][2] = {                                                      // [full][matrix]
		{{11966, 40254, 4064, 16, -6596, -22188, 28784, 28784, -26145, -2639}, {16829, 33039, 6416, 16, -9714, -19070, 28784, 28784, -24103, -4681}},
		{{13933, 46871, 4732, 0, -7509, -25259, 32768, 32768, -29763, -3005}, {19595, 38470, 7471, 0, -11058, -21710, 32768, 32768, -27439, -5329}}};
	return table[d.full][d.matrix];
}

extern "C" SMHV_API uint64_t smhv_video_bytes(uint32_t w, uint32_t h, uint32_t pixels) {
	if (w == 0 || h == 0 || w > 32768u || h > 32768u) { (void)fail(SMHV_E_INVALID, "video_bytes: %u x %u (1 .. 32768 each way)", w, h); return 0; }
	YuvDesc d;
	if (!yuv_out_decode(pixels, &d)) { (void)fail(SMHV_E_INVALID, "video_bytes: pixels 0x%x is not SMHV_PIXELS_YUV(NV12 | I420, matrix, range, 0)", pixels); return 0; }
	return yuv_tight_bytes(w, h);
}

// What both entry points share: the word, the sizes and the destination checked, `run`'s destination side and coefficients filled
// in.  Nothing is enqueued.
static int yuv_out_prepare(const char *what, uint32_t n, uint32_t w, uint32_t h, uint32_t pixels, void *d_dst, const smhv_yuv_layout *layout, YuvDesc *d, YuvOutRun *run) {
	if (!d_dst) return fail(SMHV_E_INVALID, "%s: null destination", what);
	if (n == 0 || w == 0 || h == 0 || w > 32768u || h > 32768u) return fail(SMHV_E_INVALID, "%s: %u frames of %u x %u (1 .. 32768 each way)", what, n, w, h);
	if (!yuv_out_decode(pixels, d)) return fail(SMHV_E_INVALID, "%s: pixels 0x%x is not SMHV_PIXELS_YUV(NV12 | I420, matrix, range, 0)", what, pixels);
	smhv_yuv_layout L;
	int rc = yuv_resolve_layout(what, d->layout, layout, n, w, h, &L);
	if (rc) return rc;
	if ((uint64_t)((w + 7u) / 8u) * ((h + 1u) / 2u) * n > 0x7FFFFFFFull) return fail(SMHV_E_INVALID, "%s: %u frames of %u x %u are more than one launch takes", what, n, w, h);
	*run = YuvOutRun{};
	run->dst = (uint8_t *)d_dst;
	run->y_pitch = L.y_pitch; run->uv_pitch = L.uv_pitch; run->u_off = L.u_offset; run->v_off = L.v_offset; run->dst_stride = L.frame_stride;
	run->w = w; run->h = h; run->n = n; run->k = yuv_out_coef(*d);
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_bgra_to_yuv_device(smhv_ctx *c, const void *d_src, uint64_t src_pitch_bytes, uint64_t src_stride_bytes, uint32_t n, uint32_t w, uint32_t h,
                                                uint32_t src_flags, uint32_t pixels, void *d_dst, const smhv_yuv_layout *layout, void *stream) {
	if (!c || !d_src) return fail(SMHV_E_INVALID, "bgra_to_yuv: null argument");
	if (src_flags & ~SMHV_VIDEO_SRC_RGBA) return fail(SMHV_E_INVALID, "bgra_to_yuv: unknown source flags 0x%x", src_flags);
	YuvDesc d;
	YuvOutRun run;
	int rc = yuv_out_prepare("bgra_to_yuv", n, w, h, pixels, d_dst, layout, &d, &run);
	if (rc) return rc;
	if ((uintptr_t)d_src & 3u) return fail(SMHV_E_INVALID, "bgra_to_yuv: the source is not 4-byte aligned");
	if (!src_pitch_bytes) src_pitch_bytes = 4ull * w;
	if (src_pitch_bytes < 4ull * w || (src_pitch_bytes & 3u)) return fail(SMHV_E_INVALID, "bgra_to_yuv: src_pitch_bytes %llu for rows of %llu bytes (a multiple of 4)",
	                                                                      (unsigned long long)src_pitch_bytes, 4ull * w);
	const uint64_t src_frame = src_pitch_bytes * (h - 1u) + 4ull * w;   // (the last row ends with its pixels, not with its pitch)
	if (!src_stride_bytes) src_stride_bytes = src_pitch_bytes * h;
	if ((n > 1u && src_stride_bytes < src_frame) || (src_stride_bytes & 3u)) return fail(SMHV_E_INVALID, "bgra_to_yuv: src_stride_bytes %llu, an image ends at %llu (a multiple of 4)",
	                                                                                     (unsigned long long)src_stride_bytes, (unsigned long long)src_frame);
	CTX_OPEN(c);
	HIPCHK(hipSetDevice(c->device));
	run.src = (const uint8_t *)d_src; run.src_pitch = src_pitch_bytes; run.src_stride = src_stride_bytes;
	run.rgba = (src_flags & SMHV_VIDEO_SRC_RGBA) ? 1u : 0u;
	HIPCHK(launch_bgra_to_yuv(run, d.layout, stream ? (hipStream_t)stream : c->s_main));
	return SMHV_OK;
}

extern "C" SMHV_API int smhv_batch_video(smhv_batch *b, uint32_t source, uint32_t first, uint32_t n, uint32_t pixels, void *d_dst, const smhv_yuv_layout *layout, void *stream) {
	if (!b) return fail(SMHV_E_INVALID, "batch_video: null batch");
	CTX_OPEN(b->ctx);
	if (source != SMHV_VIDEO_RENDER && source != SMHV_VIDEO_UI_MAP) return fail(SMHV_E_INVALID, "batch_video: unknown source %u", source);
	int rc = check_frames(b, first, n, "batch_video");
	if (rc) return rc;
	const Geom &g = b->g;
	const bool render = source == SMHV_VIDEO_RENDER;
	if (render && !b->d_render) return fail(SMHV_E_STATE, "batch_video: this batch has not rendered");
	if (!render && !b->ui_written) return fail(SMHV_E_STATE, "batch_video: no run of this batch has produced a ui_map (SMHV_STAGE_UI_MAP)");
	YuvDesc d;
	YuvOutRun run;
	rc = yuv_out_prepare("batch_video", n, render ? b->render_w : g.rw, render ? b->render_h : g.rh, pixels, d_dst, layout, &d, &run);
	if (rc) return rc;
	HIPCHK(hipSetDevice(b->ctx->device));
	hipStream_t s = (hipStream_t)stream;
	run.rgba = 1u;                                                // both slabs hold R, G, B, A
	if (render) {
		run.src_pitch = (uint64_t)b->render_w * 4u; run.src_stride = run.src_pitch * b->render_h;
		run.src = b->d_render + (size_t)first * run.src_stride;
		HIPCHK(hipStreamWaitEvent(s, b->ev_render, 0));           // behind the render and what drew over it, whatever stream they took
	} else {
		// Per frame the form that holds its newest ui_map (d_ui_form, as k_button left it): the luma plane -- the slab's quads, rows and
		// frames at a quarter of the pitch and stride -- or the RGBA slab.  Nothing is expanded and the batch's ui state stays as it
		// is; an expansion another reader has enqueued (it clears the flags behind it) is waited for.
		run.src = b->d_ui + (size_t)first * g.ui_stride + (size_t)g.m_xoff * 4u; run.src_pitch = g.ui_pitch; run.src_stride = g.ui_stride;
		run.luma = b->d_ui_luma + (size_t)first * (g.ui_stride / 4u) + g.m_xoff; run.luma_pitch = g.ui_pitch / 4u; run.luma_stride = g.ui_stride / 4u;
		run.form = b->d_ui_form + first;
		std::lock_guard<std::mutex> lk(b->ui_mu);
		HIPCHK(hipStreamWaitEvent(s, b->ev_ui, 0));               // (no-op before the first expansion)
	}
	HIPCHK(launch_bgra_to_yuv(run, d.layout, s));
	return SMHV_OK;
}
