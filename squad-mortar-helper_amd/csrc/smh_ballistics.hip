// smh_ballistics.hip -- ballistics: a caller-supplied weapon's firing solutions of the marker lines, and its reach map over a map view's
// window as a class byte per pixel, an f32 time-of-flight plane, a tint over the render slab and per-frame counts and extremes
// (include/smh_vision_hip.h, "ballistics": the semantics are pinned there; the solution's rule is smh_ballistics.h's, a line's source,
// range and altitude are smh_firing.h's firing_line(), a pixel's its reach_axis / reach_eval, the blend its reach_blend).
//
// k_ballistic_lines: one lane per frame, line and direction.  Both lanes of a line call firing_line() (the same loads: one round trip
//   of the wave either way), then each solves its own direction for both arcs and stores its 128-byte half of the record.
// k_ballistic_map<PAINT, PLANES> over frames x tiles of SMH_REACH_TW x SMH_REACH_TH window pixels, 256 threads: k_reach's shape.
//   Frame-uniform inputs (open, the origin, m/px, the minimap rectangle) are read once per workgroup; a frame without an origin leaves
//   at once (with PLANES its tile's plane elements are written first: class 0, a NaN time), paints nothing and counts nothing.
//   The mapping is separable: the TW + 1 columns and TH + 1 rows a tile and its +1 neighbours touch are evaluated once each, by one
//   thread each, into LDS (reach_axis).  One more thread loads the origin's texel.
//   A lane owns one column and SMH_REACH_ROWS consecutive rows.  Per pixel: reach_eval (one square root), the texel (a u16 gather), the
//   discriminant, its square root and one division for the root of the weapon's arc, nine compares for status and band, and one more
//   square root and division for the time of flight; with isochrones one division for the interval.  The isochrone rule's neighbours
//   are not evaluated again: the pixel below is the lane's next pixel, the pixel to the right is the next lane's (a shuffle of its
//   interval and source), and the column past the tile is evaluated once per wave, row i by lane i -- ROWS + 2 pixels per lane for
//   ROWS.  "No interval" travels as a NaN.
//   Counts: the lane's class bytes are kept packed; after the rows, wave ballots and popcounts, one LDS atomic per wave and count, one
//   global vector atomic per workgroup and count that is not zero.  The extremes of the time of flight: min / max over the lane's rows,
//   a wave reduction by shuffles, then as order-preserving 64-bit keys (0 = nothing yet, so the cleared slab is the identity of both)
//   one LDS and one global atomicMax each.  k_ballistic_finish, one thread per frame behind it on the stream, turns the keys into the
//   doubles.
// No scratch; every array below is indexed by unrolled constants or lies in LDS or in the kernel's arguments.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smh_firing.h"
#include "smh_ballistics.h"

namespace smh {

// ---- the lines
__global__ void __launch_bounds__(128) k_ballistic_lines(const BalLinesRun r) {
	const uint32_t f = blockIdx.y, i = blockIdx.x * 64u + (threadIdx.x >> 1), d = threadIdx.x & 1u;
	uint32_t n = r.n_lines, mm[4] = {r.mm[0], r.mm[1], r.mm[2], r.mm[3]};
	bool has_mm = r.has_mm != 0u, has_mpx = r.has_mpx != 0u;
	smhv_line ln = {0.0f, 0.0f, 0.0f, 0.0f};
	double met = 0.0;
	smhv_ballistic_solution *dst;
	if (r.per_call) {
		if (i >= n) return;
		ln = r.lines[i];
		const double ax = (double)ln.x0 - (double)ln.x1, ay = (double)ln.y0 - (double)ln.y1;   // (Marker::new, as k_firing_lines restates it)
		met = has_mpx ? sqrt(ax * ax + ay * ay) * r.mpx : 0.0;
		dst = &r.out_lines[i].dir[d];
	} else {
		if (i >= (uint32_t)SMHV_MAX_LINES) return;                   // (a slab entry holds SMHV_MAX_LINES records)
		const smhv_frame_result *res = &r.res[f];                  // (as firing_frame_tail reads the record)
		n = res->n_lines;
		has_mm = res->has_minimap != 0u; has_mpx = res->has_mpx != 0u;
		mm[0] = res->minimap[0]; mm[1] = res->minimap[1]; mm[2] = res->minimap[2]; mm[3] = res->minimap[3];
		if (i < n) { ln = res->lines[i]; met = res->meters[i]; }
		dst = &r.out[f].line[i].dir[d];
		if (threadIdx.x == 0u && blockIdx.x == 0u) { r.out[f].n_lines = n; r.out[f].reserved[0] = 0u; r.out[f].reserved[1] = 0u; r.out[f].reserved[2] = 0u; }
	}
	smhv_ballistic_solution o{};
	if (i < n) {
		const smhv_firing fl = firing_line(r.fr, has_mm, mm, ln, has_mpx, met);
		if (fl.source != SMHV_FIRING_NONE) o = bal_solve(r.w, fl.meters, d ? -fl.alt_delta : fl.alt_delta, fl.source);
	}
	*dst = o;
}

hipError_t launch_ballistic_lines(const BalLinesRun &r, uint32_t n, hipStream_t s) {
	if (n == 0u || n > 65535u) return hipErrorInvalidValue;
	if (r.per_call ? (n != 1u || r.n_lines == 0u || !r.lines || !r.out_lines) : (!r.res || !r.out)) return hipErrorInvalidValue;
	const uint32_t lines = r.per_call ? r.n_lines : (uint32_t)SMHV_MAX_LINES;
	hipLaunchKernelGGL(k_ballistic_lines, dim3((lines + 63u) / 64u, n), dim3(128), 0, s, r);
	return hipGetLastError();
}

// ---- the map
#define BAL_CNT 16u   // s_cnt: classes 1 .. 12, the isochrone pixels, pixels with a time, the source mask, spare

// a double as a 64-bit key of the same order; no double but a NaN of all ones has key 0 or ~0
__device__ __forceinline__ unsigned long long bal_key(double z) {
	const unsigned long long u = (unsigned long long)__double_as_longlong(z);
	return (u >> 63) ? ~u : u | 0x8000000000000000ull;
}
__device__ __forceinline__ double bal_unkey(unsigned long long k) {
	return __longlong_as_double((long long)((k >> 63) ? k & 0x7FFFFFFFFFFFFFFFull : ~k));
}

// One pixel: its source, its class byte without the isochrone bit, its time of flight (NaN: class 0 or 1) and its interval (NaN: none)
struct BalPixel { double tof, b; uint32_t src, cls; };
__device__ __forceinline__ BalPixel bal_pixel(const BalMapRun &r, const ReachAxis &col, const ReachAxis &row, bool has_mpx, double mpx, double h0, bool iso) {
	const ReachEval e = reach_eval(col, row, has_mpx, mpx, false, 0.0);
	BalPixel p;
	p.src = e.src; p.cls = 0u;
	p.tof = __builtin_nan(""); p.b = p.tof;
	if (e.src != SMHV_FIRING_NONE) {
		double alt = 0.0;
		if (e.src == SMHV_FIRING_HEIGHTMAP) {
			const uint16_t v = r.fr.hm[(size_t)row.ix * r.fr.hm_w + (size_t)col.ix];   // (both inside the heightmap: reach_axis)
			alt = ((double)v / 65535.0) * r.fr.zscale - h0;
		}
		const double disc = bal_disc(r.w, e.m, alt), T = bal_root(r.w, sqrt(disc), r.w.g * e.m, r.w.arc);
		p.cls = bal_class(bal_status(r.w, disc, e.m, T), bal_band(r.w, T));
		p.tof = bal_tof(r.w, e.m, T);                                // (out of range: T is NaN, and so is this)
		if (iso) p.b = floor(p.tof / r.iso_s);
	}
	return p;
}

template <bool PAINT, bool PLANES>
__global__ void __launch_bounds__(256) k_ballistic_map(const BalMapRun r) {
	__shared__ ReachAxis s_col[SMH_REACH_TW + 1u], s_row[SMH_REACH_TH + 1u];
	__shared__ double s_h0;
	__shared__ uint32_t s_cnt[BAL_CNT], s_pal[13];
	__shared__ unsigned long long s_ext[2];
	const uint32_t f = blockIdx.z, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const uint32_t x0 = blockIdx.x * SMH_REACH_TW, y0 = blockIdx.y * SMH_REACH_TH;
	const uint32_t X = x0 + lane, yb = wave * SMH_REACH_ROWS;
	const bool in_x = X < r.out_w;
	uint8_t *cls_out = PLANES && r.cls ? r.cls + (size_t)f * r.plane_stride : nullptr;
	float *tof_out = PLANES && r.tof ? r.tof + (size_t)f * r.plane_stride : nullptr;

	// ---- the frame: its origin, or none ("reach map"'s rule, as k_reach reads it)
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
		if (PLANES && in_x) {
#pragma unroll
			for (uint32_t i = 0; i < SMH_REACH_ROWS; ++i) {
				const uint32_t Y = y0 + yb + i;
				if (Y < r.out_h) {
					const size_t at = (size_t)Y * r.out_w + X;
					if (cls_out) cls_out[at] = 0u;
					if (tof_out) tof_out[at] = __builtin_nanf("");
				}
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
	if (tid < BAL_CNT) s_cnt[tid] = 0u;
	else if (tid < BAL_CNT + 2u) s_ext[tid - BAL_CNT] = 0ull;
#pragma unroll
	for (uint32_t k = 0; k < 13u; ++k)
		if (tid == 32u + k) s_pal[k] = r.pal[k];
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
	const bool iso = r.iso_s > 0.0;
	const ReachAxis col = s_col[lane];
	const double h0 = s_h0;
	// The pixel to the right is the next lane's own pixel: its source and interval come by a shuffle.  Lane 63's lies in the column past
	// the tile: lane i (< ROWS) evaluates that column's row i here, one evaluation's time for the whole wave.
	BalPixel edge = {0.0, __builtin_nan(""), SMHV_FIRING_NONE, 0u};
	if (iso) edge = bal_pixel(r, s_col[SMH_REACH_TW], s_row[yb + min(lane, SMH_REACH_ROWS - 1u)], has_mpx, mpx, h0, true);
	uint32_t packed = 0u, srcs = 0u, timed = 0u;                   // the lane's class bytes inside the window, row i in byte i; rows with a time
	double lo = __builtin_inf(), hi = -__builtin_inf();
	BalPixel own = bal_pixel(r, col, s_row[yb], has_mpx, mpx, h0, iso);
#pragma unroll
	for (uint32_t i = 0; i < SMH_REACH_ROWS; ++i) {
		const uint32_t Y = y0 + yb + i;
		BalPixel down = {0.0, __builtin_nan(""), SMHV_FIRING_NONE, 0u};
		if (iso || i + 1u < SMH_REACH_ROWS) down = bal_pixel(r, col, s_row[yb + i + 1u], has_mpx, mpx, h0, iso);
		const bool in = in_x && Y < r.out_h;
		uint32_t c = own.cls;
		if (iso) {                                                   // (uniform: every lane of the wave takes part in the shuffles)
			const double nb = __shfl_down(own.b, 1), eb = __shfl(edge.b, (int)i);
			const uint32_t ns = __shfl_down(own.src, 1), es = __shfl(edge.src, (int)i);
			const double right_b = lane == 63u ? eb : nb;
			const uint32_t right_src = lane == 63u ? es : ns;
			if (c != 0u && own.b == own.b &&
			    ((right_src == own.src && right_b == right_b && right_b != own.b) || (down.src == own.src && down.b == down.b && down.b != own.b)))
				c |= SMHV_BMAP_ISO;
		}
		const uint32_t c7 = in ? c & 0x7Fu : 0u;
		if (in) {
			const size_t at = (size_t)Y * r.out_w + X;
			packed |= c << (8u * i); srcs |= c7 ? 1u << own.src : 1u;
			if (c7 >= SMHV_BMAP_BAND0 && own.tof == own.tof) {
				timed |= 1u << i;
				lo = own.tof < lo ? own.tof : lo; hi = own.tof > hi ? own.tof : hi;
			}
			if (PLANES) {
				if (cls_out) cls_out[at] = (uint8_t)c;
				if (tof_out) tof_out[at] = (float)own.tof;
			}
			if (PAINT && c7) {
				uint32_t *p = (uint32_t *)(r.img + (size_t)f * r.img_stride) + at;
				uint32_t px = reach_blend(*p, s_pal[c7 - 1u]);
				if (c & SMHV_BMAP_ISO) px = reach_blend(px, s_pal[12]);
				*p = px;
			}
		}
		own = down;
	}

	// ---- the counts and the extremes: per wave into LDS, per workgroup into the slab (cleared ahead of the launch)
#pragma unroll
	for (uint32_t k = 0; k < 14u; ++k) {
		uint32_t cnt = 0u;
#pragma unroll
		for (uint32_t i = 0; i < SMH_REACH_ROWS; ++i) {
			const uint32_t c = (packed >> (8u * i)) & 255u;
			cnt += (uint32_t)__popcll(__ballot(k < 12u ? (c & 0x7Fu) == k + 1u : k == 12u ? (c & SMHV_BMAP_ISO) != 0u : ((timed >> i) & 1u) != 0u));
		}
		if (lane == 0u && cnt) atomicAdd(&s_cnt[k], cnt);
	}
#pragma unroll
	for (uint32_t k = 0; k < 3u; ++k) srcs |= (__ballot((srcs >> k) & 1u) != 0ull) ? 1u << k : 0u;
	if (lane == 0u && srcs) atomicOr(&s_cnt[14], srcs);
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		const double ol = __shfl_xor(lo, d), oh = __shfl_xor(hi, d);
		lo = ol < lo ? ol : lo; hi = oh > hi ? oh : hi;
	}
	if (lane == 0u && lo <= hi) {                                  // (some pixel of the wave has a time)
		atomicMax(&s_ext[0], ~bal_key(lo));
		atomicMax(&s_ext[1], bal_key(hi));
	}
	__syncthreads();
	smhv_ballistic_map_result *out = &r.out[f];
	if (tid < 12u) { if (s_cnt[tid]) atomicAdd(&out->count[tid], s_cnt[tid]); }
	else if (tid == 12u) { if (s_cnt[12]) atomicAdd(&out->iso, s_cnt[12]); }
	else if (tid == 13u) { if (s_cnt[13]) atomicAdd(&out->n_tof, s_cnt[13]); }
	else if (tid == 14u) { if (s_cnt[14]) atomicOr(&out->source_mask, s_cnt[14]); }
	else if (tid == 15u) { if (s_ext[0]) atomicMax((unsigned long long *)&out->tof_min, s_ext[0]); }
	else if (tid == 16u) { if (s_ext[1]) atomicMax((unsigned long long *)&out->tof_max, s_ext[1]); }
	else if (tid == 17u && blockIdx.x == 0u && blockIdx.y == 0u) { out->valid = 1u; out->origin[0] = ox; out->origin[1] = oy; }
}

// the extremes' keys of n summaries into their doubles (a frame without a time keeps its zeros)
__global__ void __launch_bounds__(64) k_ballistic_finish(smhv_ballistic_map_result *out, uint32_t n) {
	const uint32_t f = blockIdx.x * 64u + threadIdx.x;
	if (f >= n || out[f].n_tof == 0u) return;
	const unsigned long long kmin = ~(unsigned long long)__double_as_longlong(out[f].tof_min), kmax = (unsigned long long)__double_as_longlong(out[f].tof_max);
	out[f].tof_min = bal_unkey(kmin);
	out[f].tof_max = bal_unkey(kmax);
}

hipError_t launch_ballistic_map(const BalMapRun &r, uint32_t n, bool paint, hipStream_t s) {
	if (n == 0u || n > 65535u || r.out_w == 0u || r.out_h == 0u || !r.out || (paint && !r.img) || (!r.per_call && (!r.aux || !r.res))) return hipErrorInvalidValue;
	const bool planes = r.cls || r.tof;
	const dim3 grid((r.out_w + SMH_REACH_TW - 1u) / SMH_REACH_TW, (r.out_h + SMH_REACH_TH - 1u) / SMH_REACH_TH, n), block(256);
	if (paint && planes) hipLaunchKernelGGL((k_ballistic_map<true, true>), grid, block, 0, s, r);
	else if (paint) hipLaunchKernelGGL((k_ballistic_map<true, false>), grid, block, 0, s, r);
	else if (planes) hipLaunchKernelGGL((k_ballistic_map<false, true>), grid, block, 0, s, r);
	else hipLaunchKernelGGL((k_ballistic_map<false, false>), grid, block, 0, s, r);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_ballistic_finish, dim3((n + 63u) / 64u), dim3(64), 0, s, r.out, n);
	return hipGetLastError();
}

}  // namespace smh
