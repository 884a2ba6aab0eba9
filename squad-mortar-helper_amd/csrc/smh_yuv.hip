// smh_yuv.hip -- 8-bit 4:2:0 video frames (NV12 / I420) -> BGRA8, the layouts a video decoder leaves behind
// (include/smh_vision_hip.h, SMHV_PIXELS_NV12 / _I420; the arithmetic is pinned there).
//
// Streaming: 1.5 bytes in, 4 bytes out per pixel.  A lane converts a block of 2 rows x 4 pixels whose frame x is a multiple of 4
// and whose frame y is even, so the block shares one chroma row and two chroma columns: a dword of Y per row, a dword (NV12) or
// two half-words (I420) of chroma, two 16-byte stores.  Planes are pitched with any byte alignment, so every access has two
// forms: the wide one where the address allows it and the block lies wholly inside the rectangle, bytes / dwords otherwise.
// Bilinear chroma reads its 3 x 4 neighbourhood through the cache (adjacent lanes and the next row pair share all of it).
// A launch converts up to two rectangles of every frame (the whole frame is one rectangle), each with its own description of
// where its samples lie: the frame's planes, or the packed rows of the ingest queue's region-of-interest upload.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smh_kernels.h"

namespace smh {

// clip8(v >> 8) as clamp(v, 0, 65535) >> 8: the same value for every int.  Written this way round because hipcc fuses "shift,
// then saturate" of two channels into v_ashr_pk_u8_i32 and ORs the third channel over its result's upper half, which on the
// device was not zero: R came out wrong while B and G were right.
__device__ __forceinline__ uint32_t yuv_clip8(int v) { return (uint32_t)min(max(v, 0), 65535) >> 8; }

__device__ __forceinline__ uint32_t yuv_bgra(int Y, int U, int V, const YuvCoef &k) {
	const int c = k.cy * (Y - k.yoff), d = U - 128, e = V - 128;
	const uint32_t r = yuv_clip8(c + k.rv * e + 128);
	const uint32_t g = yuv_clip8(c - k.gu * d - k.gv * e + 128);
	const uint32_t b = yuv_clip8(c + k.bu * d + 128);
	return b | (g << 8) | (r << 16) | 0xFF000000u;
}

// one chroma sample: pu / pv = the sample's row in the U (NV12: the interleaved) and the V plane, col = its column in that row
template <int LAYOUT>
__device__ __forceinline__ void yuv_chroma(const uint8_t *pu, const uint8_t *pv, uint32_t col, int &U, int &V) {
	if (LAYOUT == SMH_YUV_NV12) {
		const uint8_t *p = pu + 2u * (size_t)col;
		if (((uintptr_t)p & 1u) == 0u) { const uint32_t w = *(const uint16_t *)p; U = (int)(w & 255u); V = (int)(w >> 8); }
		else { U = p[0]; V = p[1]; }
	} else {
		U = pu[col]; V = pv[col];
	}
}

template <int LAYOUT, int BILINEAR>
__global__ void __launch_bounds__(256) k_yuv420_to_bgra(const YuvRun run) {
	const uint32_t f = blockIdx.x / run.bands_total, b = blockIdx.x - f * run.bands_total;
	const uint32_t ri = b >= run.bands0 ? 1u : 0u;
	const YuvRect R = run.r[ri];
	const uint32_t band = ri ? b - run.bands0 : b;
	const uint8_t *src = run.src + (size_t)f * run.src_stride;
	uint8_t *dst = run.dst + (size_t)f * run.dst_stride;
	const uint32_t x_end = R.x0 + R.w, y_end = R.y0 + R.h;
	const uint32_t qx0 = R.x0 >> 2, nq = ((x_end + 3u) >> 2) - qx0;
	const uint32_t py0 = (R.y0 >> 1) + band * SMH_YUV_BAND_PAIRS, py1 = min((y_end + 1u) >> 1, py0 + SMH_YUV_BAND_PAIRS);
	const uint32_t items = (py1 - py0) * nq;
	const uint32_t cw = (run.W + 1u) >> 1, ch = (run.H + 1u) >> 1;
	const YuvCoef k = run.k;
	for (uint32_t i = threadIdx.x; i < items; i += 256u) {
		const uint32_t pr = i / nq, q = i - pr * nq;
		const uint32_t x4 = (qx0 + q) << 2, y2 = (py0 + pr) << 1;
		bool vx[4], vy[2];
#pragma unroll
		for (int j = 0; j < 4; ++j) vx[j] = x4 + j >= R.x0 && x4 + j < x_end;
#pragma unroll
		for (int r = 0; r < 2; ++r) vy[r] = y2 + r >= R.y0 && y2 + r < y_end;
		const bool full = x4 >= R.x0 && x4 + 4u <= x_end;
		int Y[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
		for (int r = 0; r < 2; ++r) {
			if (!vy[r]) continue;
			const uint8_t *p = src + R.y_off + (size_t)(y2 + r - R.y_y0) * R.y_pitch + (x4 - R.y_x0);
			if (full && ((uintptr_t)p & 3u) == 0u) {
				const uint32_t w = *(const uint32_t *)p;
				Y[r][0] = (int)(w & 255u); Y[r][1] = (int)((w >> 8) & 255u); Y[r][2] = (int)((w >> 16) & 255u); Y[r][3] = (int)(w >> 24);
			} else {
#pragma unroll
				for (int j = 0; j < 4; ++j) if (vx[j]) Y[r][j] = p[j];
			}
		}
		const uint32_t c0 = x4 >> 1, cr = y2 >> 1;
		uint32_t px[2][4];
		if (!BILINEAR) {
			int U[2] = {0, 0}, V[2] = {0, 0};
			const uint8_t *pu = src + R.u_off + (size_t)(cr - R.c_y0) * R.uv_pitch;
			const uint8_t *pv = src + R.v_off + (size_t)(cr - R.c_y0) * R.uv_pitch;
			const uint32_t col = c0 - R.c_x0;
			if (LAYOUT == SMH_YUV_NV12) {
				const uint8_t *p = pu + 2u * (size_t)col;
				if (full && ((uintptr_t)p & 3u) == 0u) {
					const uint32_t w = *(const uint32_t *)p;
					U[0] = (int)(w & 255u); V[0] = (int)((w >> 8) & 255u); U[1] = (int)((w >> 16) & 255u); V[1] = (int)(w >> 24);
				} else {
					if (vx[0] || vx[1]) { U[0] = p[0]; V[0] = p[1]; }
					if (vx[2] || vx[3]) { U[1] = p[2]; V[1] = p[3]; }
				}
			} else {
				const uint8_t *qu = pu + col, *qv = pv + col;
				if (full && (((uintptr_t)qu | (uintptr_t)qv) & 1u) == 0u) {
					const uint32_t wu = *(const uint16_t *)qu, wv = *(const uint16_t *)qv;
					U[0] = (int)(wu & 255u); U[1] = (int)(wu >> 8); V[0] = (int)(wv & 255u); V[1] = (int)(wv >> 8);
				} else {
					if (vx[0] || vx[1]) { U[0] = qu[0]; V[0] = qv[0]; }
					if (vx[2] || vx[3]) { U[1] = qu[1]; V[1] = qv[1]; }
				}
			}
#pragma unroll
			for (int r = 0; r < 2; ++r)
#pragma unroll
				for (int j = 0; j < 4; ++j) px[r][j] = yuv_bgra(Y[r][j], U[j >> 1], V[j >> 1], k);
		} else {
			// chroma rows cr - 1, cr, cr + 1 and columns c0 - 1 .. c0 + 2, clamped at the FRAME's edge; a sample is read only when a
			// pixel of the rectangle needs it (the packed rows hold no more than that)
			const uint32_t rows[3] = {cr ? cr - 1u : 0u, cr, min(cr + 1u, ch - 1u)};
			const uint32_t cols[4] = {c0 ? c0 - 1u : 0u, c0, min(c0 + 1u, cw - 1u), min(c0 + 2u, cw - 1u)};
			const bool need_r[3] = {vy[0], true, vy[1]};
			const bool need_c[4] = {vx[0], vx[0] || vx[1] || vx[2], vx[1] || vx[2] || vx[3], vx[3]};
			int U[3][4], V[3][4];
#pragma unroll
			for (int r = 0; r < 3; ++r) {
				const uint8_t *pu = src + R.u_off + (size_t)(rows[r] - R.c_y0) * R.uv_pitch;
				const uint8_t *pv = src + R.v_off + (size_t)(rows[r] - R.c_y0) * R.uv_pitch;
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					U[r][j] = 0; V[r][j] = 0;
					if (need_r[r] && need_c[j]) yuv_chroma<LAYOUT>(pu, pv, cols[j] - R.c_x0, U[r][j], V[r][j]);
				}
			}
#pragma unroll
			for (int r = 0; r < 2; ++r) {
				const int ny = r ? 2 : 0;
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					const int cx = 1 + (j >> 1), nx = j == 0 ? 0 : j == 1 ? 2 : j == 2 ? 1 : 3;
					const int u = (9 * U[1][cx] + 3 * U[1][nx] + 3 * U[ny][cx] + U[ny][nx] + 8) >> 4;
					const int v = (9 * V[1][cx] + 3 * V[1][nx] + 3 * V[ny][cx] + V[ny][nx] + 8) >> 4;
					px[r][j] = yuv_bgra(Y[r][j], u, v, k);
				}
			}
		}
#pragma unroll
		for (int r = 0; r < 2; ++r) {
			if (!vy[r]) continue;
			uint32_t *o = (uint32_t *)(dst + ((size_t)(y2 + r) * run.W + x4) * 4u);
			if (full && ((uintptr_t)o & 15u) == 0u) *(uint4 *)o = make_uint4(px[r][0], px[r][1], px[r][2], px[r][3]);
			else {
#pragma unroll
				for (int j = 0; j < 4; ++j) if (vx[j]) o[j] = px[r][j];
			}
		}
	}
}

uint32_t yuv_rect_bands(const YuvRect &r) {
	if (r.w == 0 || r.h == 0) return 0u;
	const uint32_t pairs = ((r.y0 + r.h + 1u) >> 1) - (r.y0 >> 1);
	return (pairs + SMH_YUV_BAND_PAIRS - 1u) / SMH_YUV_BAND_PAIRS;
}

// run: everything but the band counts, which are filled in here.  n_rects = 1 or 2.
hipError_t launch_yuv_to_bgra(YuvRun run, uint32_t n_rects, uint32_t layout, uint32_t bilinear, hipStream_t s) {
	run.bands0 = yuv_rect_bands(run.r[0]);
	run.bands_total = run.bands0 + (n_rects > 1u ? yuv_rect_bands(run.r[1]) : 0u);
	const uint64_t blocks = (uint64_t)run.bands_total * run.n;
	if (blocks == 0 || blocks > 0x7FFFFFFFull || (layout != SMH_YUV_NV12 && layout != SMH_YUV_I420)) return hipErrorInvalidValue;
	const dim3 grid((uint32_t)blocks), block(256);
	if (layout == SMH_YUV_NV12) {
		if (bilinear) hipLaunchKernelGGL((k_yuv420_to_bgra<SMH_YUV_NV12, 1>), grid, block, 0, s, run);
		else hipLaunchKernelGGL((k_yuv420_to_bgra<SMH_YUV_NV12, 0>), grid, block, 0, s, run);
	} else {
		if (bilinear) hipLaunchKernelGGL((k_yuv420_to_bgra<SMH_YUV_I420, 1>), grid, block, 0, s, run);
		else hipLaunchKernelGGL((k_yuv420_to_bgra<SMH_YUV_I420, 0>), grid, block, 0, s, run);
	}
	return hipGetLastError();
}

}  // namespace smh
