// smh_reach.hip -- the reach map: the firing solution from an origin to every pixel of a map view's window, as a class byte per
// pixel, a tint over the render slab and per-frame counts (include/smh_vision_hip.h, "reach map": the semantics are pinned there;
// the per-pixel rule is smh_firing.h's reach_axis / reach_eval / reach_class, firing_line()'s operations restated per axis).
//
// One kernel, k_reach<PAINT, CLASSES>, over frames x tiles of SMH_REACH_TW x SMH_REACH_TH window pixels; 256 threads.
//   Frame-uniform inputs (open, the origin, m/px, the minimap rectangle) are read once per workgroup; a frame without an origin
//   leaves at once (with CLASSES its tile's bytes are zeroed first), paints nothing and counts nothing.
//   The mapping is separable: the TW + 1 columns and TH + 1 rows a tile and its +1 neighbours touch are evaluated once each, by
//   one thread each, into LDS (ReachAxis: one f32 and two f64 divisions per entry) -- not per pixel.  One more thread loads the
//   origin's texel.
//   A lane owns one column and SMH_REACH_ROWS consecutive rows.  Per pixel: the texel (a u16 gather; lanes of a wave hit the
//   same or adjacent texels of one heightmap row), the discriminant, its square root, one division and seven compares.  A
//   pixel's range takes one f64 square root and, with rings, one division.  The ring rule's neighbours are not evaluated again:
//   the pixel below is the lane's next pixel, the pixel to the right is the next lane's (a shuffle), and the column past the
//   tile is evaluated once per wave, row i by lane i -- ROWS + 2 evaluations per lane for ROWS pixels, where three per pixel
//   would be 3 ROWS.
//   Counts: the lane's class bytes are kept packed; after the rows, wave ballots and popcounts, one LDS atomic per wave and class,
//   one global vector atomic per workgroup and class that is not zero.
// No scratch; every array below is indexed by unrolled constants or lies in LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smh_firing.h"

namespace smh {

#define RCH_CNT 12u   // s_cnt: classes 1 .. 9, the ring pixels, the source mask, spare

template <bool PAINT, bool CLASSES>
__global__ void __launch_bounds__(256) k_reach(const ReachRun r) {
	__shared__ ReachAxis s_col[SMH_REACH_TW + 1u], s_row[SMH_REACH_TH + 1u];
	__shared__ double s_h0;
	__shared__ uint32_t s_cnt[RCH_CNT], s_pal[10];
	const uint32_t f = blockIdx.z, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const uint32_t x0 = blockIdx.x * SMH_REACH_TW, y0 = blockIdx.y * SMH_REACH_TH;
	const uint32_t X = x0 + lane, yb = wave * SMH_REACH_ROWS;
	const bool in_x = X < r.out_w;
	uint8_t *cls_out = CLASSES ? r.cls + (size_t)f * r.cls_stride : nullptr;

	// ---- the frame: its origin, or none
	bool have = true, has_mm = r.has_mm != 0u, has_mpx = r.has_mpx != 0u;
	double mpx = r.mpx;
	float ox = r.origin[0], oy = r.origin[1];
	uint32_t mm[4] = {r.mm[0], r.mm[1], r.mm[2], r.mm[3]};
	if (!r.per_call) {
		const smhv_frame_result *res = &r.res[f];
		have = r.aux[f].open != 0u;
		if (have && r.origin_mode != SMHV_REACH_ORIGIN_POINT) {
			have = res->n_lines > r.line;
			if (have) {
				const smhv_line ln = res->lines[r.line];
				ox = r.origin_mode == SMHV_REACH_ORIGIN_LINE_P0 ? ln.x0 : ln.x1;
				oy = r.origin_mode == SMHV_REACH_ORIGIN_LINE_P0 ? ln.y0 : ln.y1;
			}
		}
		has_mm = res->has_minimap != 0u; has_mpx = res->has_mpx != 0u;
		mpx = res->mpx;
		mm[0] = res->minimap[0]; mm[1] = res->minimap[1]; mm[2] = res->minimap[2]; mm[3] = res->minimap[3];
	}
	have = have && isfinite(ox) && isfinite(oy);
	if (!have) {                                                   // (uniform over the workgroup)
		if (CLASSES && in_x) {
#pragma unroll
			for (uint32_t i = 0; i < SMH_REACH_ROWS; ++i) {
				const uint32_t Y = y0 + yb + i;
				if (Y < r.out_h) cls_out[(size_t)Y * r.out_w + X] = 0u;
			}
		}
		return;
	}

	// ---- the tile's columns and rows, the origin's texel
	const bool use_hm = has_mm && r.fr.hm != nullptr;
	HmRect q = {0.0f, 0.0f, 0.0f, 0.0f};
	double rw = 0.0, rh = 0.0;
	if (use_hm) {
		q = hm_rect(mm, r.fr.flags, r.fr.b0x, r.fr.b0y, r.fr.hm_w, r.fr.hm_h, r.fr.sw, r.fr.sh, r.fr.tx, r.fr.ty);
		rw = (double)(q.r - q.l); rh = (double)(q.b - q.t);
	}
	if (tid < RCH_CNT) s_cnt[tid] = 0u;
#pragma unroll
	for (uint32_t k = 0; k < 10u; ++k)
		if (tid == 16u + k) s_pal[k] = r.pal[k];
	if (tid <= SMH_REACH_TW) s_col[tid] = reach_axis((float)(x0 + tid) + 0.5f, ox, r.fr.sw, r.fr.tx, use_hm, q.l, rw, r.fr.hm_w);
	else if (tid >= 128u && tid <= 128u + SMH_REACH_TH) s_row[tid - 128u] = reach_axis((float)(y0 + tid - 128u) + 0.5f, oy, r.fr.sh, r.fr.ty, use_hm, q.t, rh, r.fr.hm_h);
	else if (tid == 192u) {
		double h0 = 0.0;
		if (use_hm) {
			const int32_t ix0 = reach_origin_texel(ox, r.fr.sw, r.fr.tx, q.l, rw, r.fr.hm_w), iy0 = reach_origin_texel(oy, r.fr.sh, r.fr.ty, q.t, rh, r.fr.hm_h);
			if (ix0 >= 0 && iy0 >= 0) h0 = ((double)r.fr.hm[(size_t)iy0 * r.fr.hm_w + (size_t)ix0] / 65535.0) * r.fr.zscale;
		}
		s_h0 = h0;
	}
	__syncthreads();

	// ---- the lane's pixels, top to bottom
	const bool rings = r.ring_m > 0.0;
	const ReachAxis col = s_col[lane];
	const double h0 = s_h0;
	// The pixel to the right is the next lane's own pixel: its source and ring interval come by a shuffle.  Lane 63's lies in the
	// column past the tile: lane i (< ROWS) evaluates that column's row i here, one evaluation's time for the whole wave.
	ReachEval edge = {0.0, 0.0, SMHV_FIRING_NONE};
	if (rings) edge = reach_eval(s_col[SMH_REACH_TW], s_row[yb + min(lane, SMH_REACH_ROWS - 1u)], has_mpx, mpx, true, r.ring_m);
	uint32_t packed = 0u, srcs = 0u;                               // the lane's class bytes inside the window, row i in byte i
	ReachEval own = reach_eval(col, s_row[yb], has_mpx, mpx, rings, r.ring_m);
#pragma unroll
	for (uint32_t i = 0; i < SMH_REACH_ROWS; ++i) {
		const uint32_t Y = y0 + yb + i;
		const ReachAxis row = s_row[yb + i];
		const ReachEval down = reach_eval(col, s_row[yb + i + 1u], has_mpx, mpx, rings, r.ring_m);
		const bool in = in_x && Y < r.out_h;
		double right_b = 0.0;
		uint32_t right_src = SMHV_FIRING_NONE;
		if (rings) {                                                 // (uniform: every lane of the wave takes part in the shuffles)
			const double nb = __shfl_down(own.b, 1), eb = __shfl(edge.b, (int)i);
			const uint32_t ns = __shfl_down(own.src, 1), es = __shfl(edge.src, (int)i);
			right_b = lane == 63u ? eb : nb;
			right_src = lane == 63u ? es : ns;
		}
		uint32_t c = 0u;
		if (own.src != SMHV_FIRING_NONE) {
			double alt = 0.0;
			if (own.src == SMHV_FIRING_HEIGHTMAP) {
				const uint16_t v = r.fr.hm[(size_t)row.ix * r.fr.hm_w + (size_t)col.ix];   // (both inside the heightmap: reach_axis)
				alt = ((double)v / 65535.0) * r.fr.zscale - h0;
			}
			c = reach_class(own.m, alt);
			if (rings && ((right_src == own.src && right_b != own.b) || (down.src == own.src && down.b != own.b))) c |= SMHV_REACH_RING;
		}
		const uint32_t c7 = in ? c & 0x7Fu : 0u;
		if (in) { packed |= c << (8u * i); srcs |= c7 ? 1u << own.src : 1u; }
		if (CLASSES && in) cls_out[(size_t)Y * r.out_w + X] = (uint8_t)c;
		if (PAINT && c7) {
			uint32_t *p = (uint32_t *)(r.img + (size_t)f * r.img_stride) + (size_t)Y * r.out_w + X;
			uint32_t px = reach_blend(*p, s_pal[c7 - 1u]);
			if (c & SMHV_REACH_RING) px = reach_blend(px, s_pal[9]);
			*p = px;
		}
		own = down;
	}

	// ---- the counts: per wave into LDS, per workgroup into the slab (cleared ahead of the launch)
#pragma unroll
	for (uint32_t k = 0; k < 10u; ++k) {
		uint32_t cnt = 0u;
#pragma unroll
		for (uint32_t i = 0; i < SMH_REACH_ROWS; ++i) {
			const uint32_t c = (packed >> (8u * i)) & 255u;
			cnt += (uint32_t)__popcll(__ballot(k < 9u ? (c & 0x7Fu) == k + 1u : (c & SMHV_REACH_RING) != 0u));
		}
		if (lane == 0u && cnt) atomicAdd(&s_cnt[k], cnt);
	}
#pragma unroll
	for (uint32_t k = 0; k < 3u; ++k) srcs |= (__ballot((srcs >> k) & 1u) != 0ull) ? 1u << k : 0u;
	if (lane == 0u && srcs) atomicOr(&s_cnt[10], srcs);
	__syncthreads();
	smhv_reach_result *out = &r.out[f];
	if (tid < 9u) { if (s_cnt[tid]) atomicAdd(&out->count[tid], s_cnt[tid]); }
	else if (tid == 9u) { if (s_cnt[9]) atomicAdd(&out->ring, s_cnt[9]); }
	else if (tid == 10u) { if (s_cnt[10]) atomicOr(&out->source_mask, s_cnt[10]); }
	else if (tid == 11u && blockIdx.x == 0u && blockIdx.y == 0u) { out->valid = 1u; out->origin[0] = ox; out->origin[1] = oy; }
}

hipError_t launch_reach(const ReachRun &r, uint32_t n, bool paint, bool classes, hipStream_t s) {
	if (n == 0u || n > 65535u || r.out_w == 0u || r.out_h == 0u || !r.out || (paint && !r.img) || (classes && !r.cls) || (!r.per_call && (!r.aux || !r.res)))
		return hipErrorInvalidValue;
	const dim3 grid((r.out_w + SMH_REACH_TW - 1u) / SMH_REACH_TW, (r.out_h + SMH_REACH_TH - 1u) / SMH_REACH_TH, n), block(256);
	if (paint && classes) hipLaunchKernelGGL((k_reach<true, true>), grid, block, 0, s, r);
	else if (paint) hipLaunchKernelGGL((k_reach<true, false>), grid, block, 0, s, r);
	else if (classes) hipLaunchKernelGGL((k_reach<false, true>), grid, block, 0, s, r);
	else hipLaunchKernelGGL((k_reach<false, false>), grid, block, 0, s, r);
	return hipGetLastError();
}

}  // namespace smh
