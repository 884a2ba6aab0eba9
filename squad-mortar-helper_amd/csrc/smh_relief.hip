// smh_relief.hip -- terrain relief: the terrain height, a hillshade value and the contour bits of every pixel of a map view's window,
// as a tint over the render slab, a flag byte plane, a shade byte plane, an f32 height plane and per-frame counts and extremes
// (include/smh_vision_hip.h, "terrain relief": the semantics are pinned there; the rectangle and the coordinates are smh_firing.h's
// hm_rect / clear_coord / round_i32, the blend its reach_blend).
//
// k_relief<PAINT, PLANES> over frames x tiles of SMH_REACH_TW x SMH_REACH_TH window pixels, 256 threads: k_reach's shape.
//   Frame-uniform inputs (open, the minimap rectangle) are read once per workgroup; a frame without relief leaves at once (with PLANES
//   its tile's plane elements are zeroed first), paints nothing and counts nothing.
//   The mapping is separable: the TW + 1 columns and TH + 1 rows a tile and its +1 neighbours touch are evaluated once each, by one
//   thread each, into LDS (ReliefAxis: the two clamped taps, the weight, the inside test; one f64 division per entry).
//   A lane owns one column and SMH_REACH_ROWS consecutive rows.  A height is four u16 taps (lanes of a wave hit the same or adjacent
//   texels of two heightmap rows), three products-and-sums and one division; with contours one more division for the level.  The
//   neighbours are not evaluated again: the pixel below is the lane's next pixel, the pixel to the right is the next lane's (a
//   shuffle), and the column past the tile is evaluated once per wave, row i by lane i -- ROWS + 2 heights per lane for ROWS pixels.
//   "No height" travels as a NaN z, "no level" as a NaN L: one double each per shuffle.
//   The shade (two divisions, a square root and a third division) is skipped unless SHADES or a PAINT with a shade weight asks for
//   it, the level when interval_m == 0, the index contour's two divisions unless a pair crosses.
//   Counts: the lane's flag bytes are kept packed; after the rows, wave ballots and popcounts, one LDS atomic per wave and count, one
//   global vector atomic per workgroup and count that is not zero.  The extremes: min / max over the lane's rows, a wave reduction by
//   shuffles, then as order-preserving 64-bit keys (0 = nothing yet, so the cleared slab is the identity of both) one LDS and one
//   global atomicMax each.  k_relief_finish, one thread per frame behind k_relief on the stream, turns the keys into the doubles.
// No scratch; every array below is indexed by unrolled constants or lies in LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smh_firing.h"

namespace smh {

// One axis of a pixel at centre c (cx or cy): r0 / rlen = the heightmap rectangle's near edge and its length, n = the heightmap's
// texels on this axis.  in: the rounded coordinate lies in [0, n).  Bilinear: i0, i1 = floor(p) and floor(p) + 1, clamped, f = the
// fraction (NaN for a NaN p: no height comes of it).  Nearest: i0 = the rounded coordinate.  Both taps lie in [0, n) whenever in is set.
struct ReliefAxis { double f; int32_t i0, i1; uint32_t in, pad; };
__device__ __forceinline__ ReliefAxis relief_axis(float c, float r0, double rlen, uint32_t n, bool nearest) {
	ReliefAxis a;
	const double p = clear_coord(c, r0, rlen, n);
	const int32_t ri = round_i32(p), N = (int32_t)n;
	a.in = ri >= 0 && ri < N ? 1u : 0u;
	a.f = 0.0; a.i0 = 0; a.i1 = 0; a.pad = 0u;
	if (a.in) {
		if (nearest) { a.i0 = ri; a.i1 = ri; }
		else if (p == p) {                                           // (inside: -0.5 <= p < n - 0.5, so floor(p) is -1 .. n - 1)
			const double fl = floor(p);
			const int32_t i = (int32_t)fl;
			a.f = p - fl;
			a.i0 = min(max(i, 0), N - 1); a.i1 = min(max(i + 1, 0), N - 1);
		} else a.f = p;
	}
	return a;
}

// the height of the pixel of column c and row r; NaN: it has none
__device__ __forceinline__ double relief_z(const ReliefAxis &c, const ReliefAxis &r, const uint16_t *hm, uint32_t hm_w, double zscale, bool nearest) {
	const double none = __builtin_nan("");
	if (!(c.in & r.in)) return none;
	const uint16_t *r0 = hm + (size_t)r.i0 * hm_w, *r1 = hm + (size_t)r.i1 * hm_w;
	double z;
	if (nearest) z = clear_height(r0[c.i0], zscale);
	else {
		const double v00 = (double)r0[c.i0], v10 = (double)r0[c.i1], v01 = (double)r1[c.i0], v11 = (double)r1[c.i1];
		const double gx = 1.0 - c.f, gy = 1.0 - r.f;
		const double top = v00 * gx + v10 * c.f, bot = v01 * gx + v11 * c.f;
		const double v = top * gy + bot * r.f;
		z = (v / 65535.0) * zscale;
	}
	return isfinite(z) ? z : none;
}
// L of a height (NaN: none)
__device__ __forceinline__ double relief_level(double z, double base_m, double interval_m) {
	return z == z ? floor((z - base_m) / interval_m) : z;
}
// SMHV_RELIEF_CONTOUR | SMHV_RELIEF_MAJOR of one pair of levels, 0 when it does not cross
__device__ __forceinline__ uint32_t relief_pair(double a, double b, uint32_t major_every) {
	if (!(isfinite(a) && isfinite(b) && a != b)) return 0u;
	uint32_t bits = SMHV_RELIEF_CONTOUR;
	if (major_every) {
		const double lo = a < b ? a : b, hi = a < b ? b : a, m = (double)major_every;
		if (floor(hi / m) != floor(lo / m)) bits |= SMHV_RELIEF_MAJOR;
	}
	return bits;
}
// a double as a 64-bit key of the same order; no finite double has key 0 or ~0
__device__ __forceinline__ unsigned long long relief_key(double z) {
	const unsigned long long u = (unsigned long long)__double_as_longlong(z);
	return (u >> 63) ? ~u : u | 0x8000000000000000ull;
}
__device__ __forceinline__ double relief_unkey(unsigned long long k) {
	return __longlong_as_double((long long)((k >> 63) ? k & 0x7FFFFFFFFFFFFFFFull : ~k));
}

template <bool PAINT, bool PLANES>
__global__ void __launch_bounds__(256) k_relief(const ReliefRun r) {
	__shared__ ReliefAxis s_col[SMH_REACH_TW + 1u], s_row[SMH_REACH_TH + 1u];
	__shared__ uint32_t s_cnt[4];
	__shared__ unsigned long long s_ext[2];
	const uint32_t f = blockIdx.z, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const uint32_t x0 = blockIdx.x * SMH_REACH_TW, y0 = blockIdx.y * SMH_REACH_TH;
	const uint32_t X = x0 + lane, yb = wave * SMH_REACH_ROWS;
	const bool in_x = X < r.out_w;
	uint8_t *bytes_out = PLANES && r.bytes ? r.bytes + (size_t)f * r.plane_stride : nullptr;
	uint8_t *shades_out = PLANES && r.shades ? r.shades + (size_t)f * r.plane_stride : nullptr;
	float *heights_out = PLANES && r.heights ? r.heights + (size_t)f * r.plane_stride : nullptr;

	// ---- the frame: its minimap rectangle, or none
	bool have = r.has_mm != 0u;
	uint32_t mm[4] = {r.mm[0], r.mm[1], r.mm[2], r.mm[3]};
	if (!r.per_call) {
		const smhv_frame_result *res = &r.res[f];
		have = r.aux[f].open != 0u && res->has_minimap != 0u;
		mm[0] = res->minimap[0]; mm[1] = res->minimap[1]; mm[2] = res->minimap[2]; mm[3] = res->minimap[3];
	}
	if (!have) {                                                   // (uniform over the workgroup)
		if (PLANES && in_x) {
#pragma unroll
			for (uint32_t i = 0; i < SMH_REACH_ROWS; ++i) {
				const uint32_t Y = y0 + yb + i;
				if (Y < r.out_h) {
					const size_t at = (size_t)Y * r.out_w + X;
					if (bytes_out) bytes_out[at] = 0u;
					if (shades_out) shades_out[at] = 0u;
					if (heights_out) heights_out[at] = 0.0f;
				}
			}
		}
		return;
	}

	// ---- the tile's columns and rows
	const bool nearest = r.nearest != 0u;
	const HmRect q = hm_rect(mm, r.fr.flags, r.fr.b0x, r.fr.b0y, r.fr.hm_w, r.fr.hm_h, r.fr.sw, r.fr.sh, r.fr.tx, r.fr.ty);
	const double rw = (double)(q.r - q.l), rh = (double)(q.b - q.t);
	if (tid < 4u) s_cnt[tid] = 0u;
	else if (tid < 6u) s_ext[tid - 4u] = 0ull;
	if (tid <= SMH_REACH_TW) s_col[tid] = relief_axis((float)(x0 + tid) + 0.5f, q.l, rw, r.fr.hm_w, nearest);
	else if (tid >= 128u && tid <= 128u + SMH_REACH_TH) s_row[tid - 128u] = relief_axis((float)(y0 + tid - 128u) + 0.5f, q.t, rh, r.fr.hm_h, nearest);
	__syncthreads();

	// ---- the lane's pixels, top to bottom
	const bool levels = r.interval_m > 0.0;
	const bool shading = (PLANES && shades_out) || (PAINT && r.shade_weight != 0u);
	const double mx = (double)r.fr.hm_w / rw, my = (double)r.fr.hm_h / rh;
	const ReliefAxis col = s_col[lane];
	// The pixel to the right is the next lane's own pixel: its height and level come by a shuffle.  Lane 63's lies in the column past
	// the tile: lane i (< ROWS) evaluates that column's row i here, one evaluation's time for the whole wave.
	const double edge_z = relief_z(s_col[SMH_REACH_TW], s_row[yb + min(lane, SMH_REACH_ROWS - 1u)], r.fr.hm, r.fr.hm_w, r.fr.zscale, nearest);
	const double edge_l = levels ? relief_level(edge_z, r.base_m, r.interval_m) : edge_z;
	uint32_t packed = 0u;                                          // the lane's flag bytes inside the window, row i in byte i
	double lo = __builtin_inf(), hi = -__builtin_inf();
	double own_z = relief_z(col, s_row[yb], r.fr.hm, r.fr.hm_w, r.fr.zscale, nearest);
	double own_l = levels ? relief_level(own_z, r.base_m, r.interval_m) : own_z;
#pragma unroll
	for (uint32_t i = 0; i < SMH_REACH_ROWS; ++i) {
		const uint32_t Y = y0 + yb + i;
		const double down_z = relief_z(col, s_row[yb + i + 1u], r.fr.hm, r.fr.hm_w, r.fr.zscale, nearest);
		const double down_l = levels ? relief_level(down_z, r.base_m, r.interval_m) : down_z;
		const bool in = in_x && Y < r.out_h, has = own_z == own_z;
		uint32_t bits = has ? SMHV_RELIEF_HAS_HEIGHT : 0u;
		if (levels) {                                                // (uniform: every lane of the wave takes part in the shuffles)
			const double nl = __shfl_down(own_l, 1), el = __shfl(edge_l, (int)i);
			bits |= relief_pair(own_l, lane == 63u ? el : nl, r.major_every) | relief_pair(own_l, down_l, r.major_every);
		}
		uint32_t shade = 0u;
		if (shading) {                                               // (uniform likewise)
			const double nz = __shfl_down(own_z, 1), ez = __shfl(edge_z, (int)i);
			const double right_z = lane == 63u ? ez : nz;
			if (has) {
				const double p = right_z == right_z ? ((right_z - own_z) * r.exaggeration) / mx : 0.0;
				const double w = down_z == down_z ? ((down_z - own_z) * r.exaggeration) / my : 0.0;
				const double t = (r.light[2] - p * r.light[0]) - w * r.light[1];
				const double den = sqrt((1.0 + p * p) + w * w);
				double s = t / den;
				if (!(s > 0.0)) s = 0.0;
				if (s > 1.0) s = 1.0;
				shade = (uint32_t)(uint8_t)(s * 255.0 + 0.5);
			}
		}
		if (in) {
			const size_t at = (size_t)Y * r.out_w + X;
			packed |= bits << (8u * i);
			if (has) { lo = own_z < lo ? own_z : lo; hi = own_z > hi ? own_z : hi; }
			if (PLANES) {
				if (bytes_out) bytes_out[at] = (uint8_t)bits;
				if (shades_out) shades_out[at] = (uint8_t)shade;
				if (heights_out) heights_out[at] = has ? (float)own_z : 0.0f;
			}
			if (PAINT && has) {
				uint32_t *p = (uint32_t *)(r.img + (size_t)f * r.img_stride) + at;
				uint32_t px = reach_blend(*p, shade * 0x010101u | (r.shade_weight << 24));
				if (bits & SMHV_RELIEF_CONTOUR) px = reach_blend(px, (bits & SMHV_RELIEF_MAJOR) ? r.pal[1] : r.pal[0]);
				*p = px;
			}
		}
		own_z = down_z; own_l = down_l;
	}

	// ---- the counts and the extremes: per wave into LDS, per workgroup into the slab (cleared ahead of the launch)
#pragma unroll
	for (uint32_t k = 0; k < 3u; ++k) {
		uint32_t cnt = 0u;
#pragma unroll
		for (uint32_t i = 0; i < SMH_REACH_ROWS; ++i) cnt += (uint32_t)__popcll(__ballot((packed >> (8u * i + k)) & 1u));
		if (lane == 0u && cnt) atomicAdd(&s_cnt[k], cnt);
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		const double ol = __shfl_xor(lo, d), oh = __shfl_xor(hi, d);
		lo = ol < lo ? ol : lo; hi = oh > hi ? oh : hi;
	}
	if (lane == 0u && lo <= hi) {                                  // (some pixel of the wave has a height)
		atomicMax(&s_ext[0], ~relief_key(lo));
		atomicMax(&s_ext[1], relief_key(hi));
	}
	__syncthreads();
	smhv_relief_result *out = &r.out[f];
	if (tid == 0u) { if (s_cnt[0]) atomicAdd(&out->n_height, s_cnt[0]); }
	else if (tid == 1u) { if (s_cnt[1]) atomicAdd(&out->n_contour, s_cnt[1]); }
	else if (tid == 2u) { if (s_cnt[2]) atomicAdd(&out->n_major, s_cnt[2]); }
	else if (tid == 3u) { if (s_ext[0]) atomicMax((unsigned long long *)&out->z_min, s_ext[0]); }
	else if (tid == 4u) { if (s_ext[1]) atomicMax((unsigned long long *)&out->z_max, s_ext[1]); }
	else if (tid == 5u && blockIdx.x == 0u && blockIdx.y == 0u) out->valid = 1u;
}

// the extremes' keys of n summaries into their doubles (a frame without a height keeps its zeros)
__global__ void __launch_bounds__(64) k_relief_finish(smhv_relief_result *out, uint32_t n) {
	const uint32_t f = blockIdx.x * 64u + threadIdx.x;
	if (f >= n || out[f].n_height == 0u) return;
	const unsigned long long kmin = ~(unsigned long long)__double_as_longlong(out[f].z_min), kmax = (unsigned long long)__double_as_longlong(out[f].z_max);
	out[f].z_min = relief_unkey(kmin);
	out[f].z_max = relief_unkey(kmax);
}

hipError_t launch_relief(const ReliefRun &r, uint32_t n, bool paint, hipStream_t s) {
	if (n == 0u || n > 65535u || r.out_w == 0u || r.out_h == 0u || !r.out || !r.fr.hm || r.fr.hm_w == 0u || r.fr.hm_h == 0u || (paint && !r.img) ||
	    (!r.per_call && (!r.aux || !r.res)))
		return hipErrorInvalidValue;
	const bool planes = r.bytes || r.shades || r.heights;
	const dim3 grid((r.out_w + SMH_REACH_TW - 1u) / SMH_REACH_TW, (r.out_h + SMH_REACH_TH - 1u) / SMH_REACH_TH, n), block(256);
	if (paint && planes) hipLaunchKernelGGL((k_relief<true, true>), grid, block, 0, s, r);
	else if (paint) hipLaunchKernelGGL((k_relief<true, false>), grid, block, 0, s, r);
	else if (planes) hipLaunchKernelGGL((k_relief<false, true>), grid, block, 0, s, r);
	else hipLaunchKernelGGL((k_relief<false, false>), grid, block, 0, s, r);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_relief_finish, dim3((n + 63u) / 64u), dim3(64), 0, s, r.out, n);
	return hipGetLastError();
}

}  // namespace smh
