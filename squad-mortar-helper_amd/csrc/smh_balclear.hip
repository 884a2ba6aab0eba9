// smh_balclear.hip -- ballistic clearance: the heightmap sampled along a line of fire, held against BOTH arcs of a caller-supplied weapon
// and the straight sight line (include/smh_vision_hip.h, "ballistic clearance": the semantics are pinned there; the end points, the
// texels and the heights are smh_firing.h's clear_coord / clear_texel / clear_height, the per-arc steps smh_ballistics.h's
// bal_clear_arc / bal_clear_sample, shared by both kernels and by tests/ballistic_clearance_rule_check.cpp).
//
// k_bclear_lines: k_clear_lines' shape -- one wave per (frame, line, direction), two waves per workgroup, the lanes stride the interior
//   samples.  A lane evaluates both arcs from one texel, one height and one x; counts come from ballots, (min_margin, min_at) and
//   first_blocked per arc from the same total-order butterfly.  Lane 0 writes the 96-byte record.
// k_bclear_map<PAINT, PLANES>: k_clear_map's 64 x 16 tiles, its LDS staging of SMH_CLEAR_KC samples (t, the texel column per tile
//   column, the texel row per tile row) and its one-sample-ahead u16 gathers.  The two arcs share everything up to w.g * (x * x); the
//   last six operations (one true division each) and the flags are per arc.  A lane keeps, per pixel, d, alt, two roots, two 1 + T * T
//   and the own arc's running minimum -- fourteen registers against k_clear_map's ten -- so a lane owns SMH_BCLR_ROWS = 2 rows, not
//   four, and a tile is eight waves: 112 - 121 VGPRs, four waves per SIMD as k_clear_map has, and nothing spills (with four rows the
//   forms that write planes take 129 - 136 and lose a wave; the march is not unrolled: unrolled by two it spills SGPRs).  What the march
//   does not change of a pixel (verdict, no arc, unusable arcs) travels as bits of one register.  Nobody leaves the march early.
//   Counts: ballots, one LDS atomic per wave and count, one global vector atomic per workgroup and count that is not zero.
// No scratch; every array below is indexed by unrolled constants or lies in LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smh_firing.h"
#include "smh_ballistics.h"

namespace smh {

#define BCLR_NO_K 0xFFFFFFFFu   // min_at while no sample has replaced the starting +inf

__global__ void __launch_bounds__(128) k_bclear_lines(const BalClearLinesRun r) {
	const uint32_t l = blockIdx.x, f = blockIdx.y, lane = threadIdx.x & 63u, dir = threadIdx.x >> 6;
	const uint32_t S = r.samples;
	// ---- the line and where its results go
	bool live, has_mm;
	uint32_t mm[4];
	smhv_line ln = {0.0f, 0.0f, 0.0f, 0.0f};
	smhv_ballistic_clearance_dir *out;
	if (r.per_call) {
		live = l < r.n_lines;
		if (!live) return;
		ln = r.lines[l];
		has_mm = r.has_mm != 0u;
		mm[0] = r.mm[0]; mm[1] = r.mm[1]; mm[2] = r.mm[2]; mm[3] = r.mm[3];
		out = &r.out_lines[l].dir[dir];
	} else {
		const smhv_frame_result *res = &r.res[f];
		const uint32_t n = res->n_lines;
		live = l < n;
		if (live) ln = res->lines[l];
		has_mm = res->has_minimap != 0u;
		mm[0] = res->minimap[0]; mm[1] = res->minimap[1]; mm[2] = res->minimap[2]; mm[3] = res->minimap[3];
		out = &r.out[f].line[l].dir[dir];
		if (l == 0u && threadIdx.x == 0u) { r.out[f].n_lines = n; r.out[f].reserved[0] = 0u; r.out[f].reserved[1] = 0u; r.out[f].reserved[2] = 0u; }
	}

	// ---- the end points: "terrain clearance"'s, which are firing_line()'s heightmap branch
	bool ok = false;
	double x0 = 0.0, y0 = 0.0, x1 = 0.0, y1 = 0.0, d = 0.0, h0 = 0.0, h1 = 0.0;
	const FiringRun &fr = r.fr;
	if (live && has_mm && fr.hm) {
		const float p0x = ln.x0 * fr.sw + fr.tx, p0y = ln.y0 * fr.sh + fr.ty;
		const float p1x = ln.x1 * fr.sw + fr.tx, p1y = ln.y1 * fr.sh + fr.ty;
		const HmRect q = hm_rect(mm, fr.flags, fr.b0x, fr.b0y, fr.hm_w, fr.hm_h, fr.sw, fr.sh, fr.tx, fr.ty);
		const double rw = (double)(q.r - q.l), rh = (double)(q.b - q.t);
		x0 = clear_coord(p0x, q.l, rw, fr.hm_w); y0 = clear_coord(p0y, q.t, rh, fr.hm_h);
		x1 = clear_coord(p1x, q.l, rw, fr.hm_w); y1 = clear_coord(p1y, q.t, rh, fr.hm_h);
		const double dx = x0 - x1, dy = y0 - y1;
		d = sqrt(dx * dx + dy * dy);
		const int32_t ix0 = round_i32(x0), iy0 = round_i32(y0), ix1 = round_i32(x1), iy1 = round_i32(y1);
		const int32_t W = (int32_t)fr.hm_w, H = (int32_t)fr.hm_h;
		ok = ix0 >= 0 && iy0 >= 0 && ix1 >= 0 && iy1 >= 0 && ix0 < W && iy0 < H && ix1 < W && iy1 < H;
		if (ok) {
			const uint16_t v0 = fr.hm[(size_t)iy0 * fr.hm_w + (size_t)ix0], v1 = fr.hm[(size_t)iy1 * fr.hm_w + (size_t)ix1];
			h0 = clear_height(v0, fr.zscale); h1 = clear_height(v1, fr.zscale);
		}
	}
	if (!ok) {                                                     // (uniform over the wave) no verdict: zeros
		if (lane == 0u) *out = smhv_ballistic_clearance_dir{};
		return;
	}
	double alt = h1 - h0;
	if (dir != 0u) {                                               // the line (P1, P0)
		double s;
		s = x0; x0 = x1; x1 = s;
		s = y0; y0 = y1; y1 = s;
		h0 = h1;
		alt = -alt;
	}
	const smhv_weapon_rule &w = r.w;
	const double disc = bal_disc(w, d, alt), sq = sqrt(disc), gm = w.g * d, den = 2.0 * w.v2;
	const BalClearArc arc[2] = {bal_clear_arc(w, disc, sq, gm, d, SMHV_ARC_HIGH), bal_clear_arc(w, disc, sq, gm, d, SMHV_ARC_LOW)};
	const bool oor = !(disc >= 0.0), none = d == 0.0;              // no arc / no samples

	// ---- the interior samples, 64 at a time: one texel, one height and one x serve both arcs
	uint32_t n_blocked[2] = {0u, 0u}, first[2] = {S, S}, at[2] = {BCLR_NO_K, BCLR_NO_K}, n_los = 0u;
	double best[2] = {__builtin_inf(), __builtin_inf()};
	for (uint32_t base = 1u; base < S; base += 64u) {
		const uint32_t k = base + lane;
		const bool act = k < S && !none;
		const double t = (double)k / (double)S;
		const uint32_t sx = clear_texel(x0, x1, t, fr.hm_w), sy = clear_texel(y0, y1, t, fr.hm_h);
		const double z = clear_height(fr.hm[(size_t)sy * fr.hm_w + (size_t)sx], fr.zscale) - h0;   // (clamped: in bounds for every lane)
		const double x = d * t, gxx = w.g * (x * x);
		n_los += (uint32_t)__popcll(__ballot(act && bal_clear_los(alt, t, z)));
#pragma unroll
		for (uint32_t a = 0; a < 2u; ++a) {
			const double m = bal_clear_sample(x, gxx, arc[a].T, arc[a].qq1, den, z);
			const bool blk = act && !oor && m < r.margin_m;
			n_blocked[a] += (uint32_t)__popcll(__ballot(blk));
			if (blk) first[a] = min(first[a], k);
			if (act && !oor && m < best[a]) { best[a] = m; at[a] = k; }
		}
	}
#pragma unroll
	for (int off = 32; off; off >>= 1) {
#pragma unroll
		for (uint32_t a = 0; a < 2u; ++a) {
			const double ob = __shfl_xor(best[a], off);
			const uint32_t oa = __shfl_xor(at[a], off);
			if (ob < best[a] || (ob == best[a] && oa < at[a])) { best[a] = ob; at[a] = oa; }
			first[a] = min(first[a], (uint32_t)__shfl_xor(first[a], off));
		}
	}
	if (lane == 0u) {
		smhv_ballistic_clearance_dir o{};
		uint32_t st[2], bal[2];
#pragma unroll
		for (uint32_t a = 0; a < 2u; ++a) {
			st[a] = bal_clear_status(oor, none, n_blocked[a] != 0u);
			bal[a] = arc[a].bal;
			o.arc[a].status = st[a];
			o.arc[a].first_blocked = first[a];
			o.arc[a].n_blocked = n_blocked[a];
			o.arc[a].bal = bal[a];
			o.arc[a].min_margin = at[a] == BCLR_NO_K ? 0.0 : bal_clear_margin(best[a]);
			o.arc[a].min_at = at[a] == BCLR_NO_K ? 0u : at[a];
			o.arc[a].reserved = 0u;
		}
		o.meters = d; o.alt_delta = alt;
		o.los_blocked = n_los;
		o.valid = 1u;
		o.choice = bal_clear_choice(w.arc, st, bal);
		o.reserved = 0u;
		*out = o;
	}
}

// the heightmap coordinate of a window pixel's target on one axis (c = the pixel's centre), and of the origin: reach_axis()'s c1, c0
__device__ __forceinline__ double bclear_target_coord(float c, float s, float t, float r0, double rlen, uint32_t n) {
	const float tg = (c - t) / s;                                  // MapViewport::inverse_xy
	const float p1 = tg * s + t;                                   // MapViewport::translate_xy
	return clear_coord(p1, r0, rlen, n);
}
__device__ __forceinline__ double bclear_origin_coord(float o, float s, float t, float r0, double rlen, uint32_t n) {
	const float p0 = o * s + t;
	return clear_coord(p0, r0, rlen, n);
}

#define BCLR_F_VERDICT 1u   // a pixel's flags: a verdict exists, no arc, the own / the other arc's bal is not 0
#define BCLR_F_OOR 2u
#define BCLR_F_UNUS0 4u
#define BCLR_F_UNUS1 8u
#define BCLR_CNT 10u   // s_cnt: own classes 1 .. 4, other classes 1 .. 4, LOS pixels, switch pixels

template <bool PAINT, bool PLANES>
__global__ void __launch_bounds__(SMH_BCLR_THREADS) k_bclear_map(const BalClearMapRun r) {
	__shared__ ReachAxis s_col[SMH_REACH_TW], s_row[SMH_REACH_TH];
	__shared__ double s_c1x[SMH_REACH_TW], s_c1y[SMH_REACH_TH];    // the targets' own heightmap coordinates
	__shared__ double s_org[3];                                    // the origin's heightmap coordinates and its height
	__shared__ double s_t[SMH_CLEAR_KC];                           // the staged samples: t ...
	__shared__ uint32_t s_cx[SMH_CLEAR_KC][SMH_REACH_TW];          //   ... the texel column of each tile column ...
	__shared__ uint32_t s_ry[SMH_CLEAR_KC][SMH_REACH_TH];          //   ... and the texel row of each tile row, times the heightmap's width
	__shared__ uint32_t s_cnt[BCLR_CNT], s_pal[6];
	const uint32_t f = blockIdx.z, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const uint32_t px0 = blockIdx.x * SMH_REACH_TW, py0 = blockIdx.y * SMH_REACH_TH;
	const uint32_t X = px0 + lane, yb = wave * SMH_BCLR_ROWS;
	const bool in_x = X < r.out_w;
	uint8_t *bytes_out = PLANES && r.bytes ? r.bytes + (size_t)f * r.plane_stride : nullptr;
	float *margin_out = PLANES && r.margin ? r.margin + (size_t)f * r.plane_stride : nullptr;

	// ---- the frame: its origin, or none (k_reach's rule)
	bool have = true, has_mm = r.has_mm != 0u;
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
		has_mm = res->has_minimap != 0u;
		mm[0] = res->minimap[0]; mm[1] = res->minimap[1]; mm[2] = res->minimap[2]; mm[3] = res->minimap[3];
	}
	have = have && isfinite(ox) && isfinite(oy);
	if (!have) {                                                   // (uniform over the workgroup)
		if (PLANES && in_x) {
#pragma unroll
			for (uint32_t i = 0; i < SMH_BCLR_ROWS; ++i) {
				const uint32_t Y = py0 + yb + i;
				if (Y < r.out_h) {
					const size_t at = (size_t)Y * r.out_w + X;
					if (bytes_out) bytes_out[at] = 0u;
					if (margin_out) margin_out[at] = __builtin_nanf("");
				}
			}
		}
		return;
	}

	// ---- the tile's columns and rows, the origin
	const FiringRun &fr = r.fr;
	const smhv_weapon_rule &w = r.w;
	const bool use_hm = has_mm && fr.hm != nullptr;
	HmRect q = {0.0f, 0.0f, 0.0f, 0.0f};
	double rw = 0.0, rh = 0.0;
	if (use_hm) {
		q = hm_rect(mm, fr.flags, fr.b0x, fr.b0y, fr.hm_w, fr.hm_h, fr.sw, fr.sh, fr.tx, fr.ty);
		rw = (double)(q.r - q.l); rh = (double)(q.b - q.t);
	}
	if (tid < BCLR_CNT) s_cnt[tid] = 0u;
	else if (tid < BCLR_CNT + 6u) s_pal[tid - BCLR_CNT] = r.pal[tid - BCLR_CNT];
	if (tid >= 64u && tid < 64u + SMH_REACH_TW) {
		const uint32_t e = tid - 64u;
		const float c = (float)(px0 + e) + 0.5f;
		s_col[e] = reach_axis(c, ox, fr.sw, fr.tx, use_hm, q.l, rw, fr.hm_w);
		s_c1x[e] = use_hm ? bclear_target_coord(c, fr.sw, fr.tx, q.l, rw, fr.hm_w) : 0.0;
	} else if (tid >= 128u && tid < 128u + SMH_REACH_TH) {
		const uint32_t e = tid - 128u;
		const float c = (float)(py0 + e) + 0.5f;
		s_row[e] = reach_axis(c, oy, fr.sh, fr.ty, use_hm, q.t, rh, fr.hm_h);
		s_c1y[e] = use_hm ? bclear_target_coord(c, fr.sh, fr.ty, q.t, rh, fr.hm_h) : 0.0;
	} else if (tid == 192u) {
		double c0x = 0.0, c0y = 0.0, h0 = 0.0;
		if (use_hm) {
			c0x = bclear_origin_coord(ox, fr.sw, fr.tx, q.l, rw, fr.hm_w); c0y = bclear_origin_coord(oy, fr.sh, fr.ty, q.t, rh, fr.hm_h);
			const int32_t ix0 = reach_origin_texel(ox, fr.sw, fr.tx, q.l, rw, fr.hm_w), iy0 = reach_origin_texel(oy, fr.sh, fr.ty, q.t, rh, fr.hm_h);
			if (ix0 >= 0 && iy0 >= 0) h0 = clear_height(fr.hm[(size_t)iy0 * fr.hm_w + (size_t)ix0], fr.zscale);
		}
		s_org[0] = c0x; s_org[1] = c0y; s_org[2] = h0;
	}
	__syncthreads();

	// ---- the lane's pixels: the weapon terms of both arcs, the own arc first
	const ReachAxis col = s_col[lane];
	const double c0x = s_org[0], c0y = s_org[1], h0 = s_org[2], den = 2.0 * w.v2;
	const uint32_t own_arc = w.arc, oth_arc = 1u - w.arc;
	double d[SMH_BCLR_ROWS], alt[SMH_BCLR_ROWS], T[SMH_BCLR_ROWS][2], qq1[SMH_BCLR_ROWS][2], best[SMH_BCLR_ROWS];
	uint32_t fl[SMH_BCLR_ROWS];                                    // what the march does not change, as bits (BCLR_F_*): a register, not four lane masks
	bool blk[SMH_BCLR_ROWS][2], los[SMH_BCLR_ROWS];
#pragma unroll
	for (uint32_t i = 0; i < SMH_BCLR_ROWS; ++i) {
		const ReachAxis row = s_row[yb + i];
		const bool verdict = col.ix >= 0 && row.ix >= 0;              // the heightmap branch: the origin and the target inside
		const uint16_t v = verdict ? fr.hm[(size_t)row.ix * fr.hm_w + (size_t)col.ix] : (uint16_t)0u;
		const double dx = col.dh, dy = row.dh;
		d[i] = sqrt(dx * dx + dy * dy);
		alt[i] = clear_height(v, fr.zscale) - h0;
		const double disc = bal_disc(w, d[i], alt[i]), sq = sqrt(disc), gm = w.g * d[i];
		const BalClearArc a0 = bal_clear_arc(w, disc, sq, gm, d[i], own_arc), a1 = bal_clear_arc(w, disc, sq, gm, d[i], oth_arc);
		T[i][0] = a0.T; qq1[i][0] = a0.qq1;
		T[i][1] = a1.T; qq1[i][1] = a1.qq1;
		fl[i] = (verdict ? BCLR_F_VERDICT : 0u) | (!(disc >= 0.0) ? BCLR_F_OOR : 0u) | (a0.bal ? BCLR_F_UNUS0 : 0u) | (a1.bal ? BCLR_F_UNUS1 : 0u);
		best[i] = __builtin_inf();
		blk[i][0] = false; blk[i][1] = false; los[i] = false;
	}

	// ---- the march: SMH_CLEAR_KC samples staged, then walked by every lane
	const uint32_t S = r.samples, n_int = use_hm ? S - 1u : 0u;       // interior samples (none without a heightmap: no verdict anywhere)
	for (uint32_t base = 0; base < n_int; base += SMH_CLEAR_KC) {
		if (base) __syncthreads();                                 // (the previous samples have been read)
		{
			const uint32_t j = tid / (SMH_BCLR_THREADS / SMH_CLEAR_KC), part = tid % (SMH_BCLR_THREADS / SMH_CLEAR_KC);   // sixteen threads per sample
			const double t = (double)(1u + base + j) / (double)S;
			if (part == 0u) s_t[j] = t;
			for (uint32_t e = part; e < SMH_REACH_TW + SMH_REACH_TH; e += SMH_BCLR_THREADS / SMH_CLEAR_KC) {
				if (e < SMH_REACH_TW) s_cx[j][e] = clear_texel(c0x, s_c1x[e], t, fr.hm_w);
				else s_ry[j][e - SMH_REACH_TW] = clear_texel(c0y, s_c1y[e - SMH_REACH_TW], t, fr.hm_h) * fr.hm_w;
			}
		}
		__syncthreads();
		const uint32_t nk = min(SMH_CLEAR_KC, n_int - base);
		// the texels of sample j + 1 are on their way while sample j is held against the arcs (the last sample asks for its own again)
		uint16_t v[SMH_BCLR_ROWS];
#pragma unroll
		for (uint32_t i = 0; i < SMH_BCLR_ROWS; ++i) v[i] = fr.hm[(size_t)(s_ry[0][yb + i] + s_cx[0][lane])];   // (w * h <= 2^28; clamped: in bounds for every lane)
#pragma unroll 1
		for (uint32_t j = 0; j < nk; ++j) {
			const double t = s_t[j];
			const uint32_t jn = min(j + 1u, nk - 1u), cx = s_cx[jn][lane];
			uint16_t vn[SMH_BCLR_ROWS];
#pragma unroll
			for (uint32_t i = 0; i < SMH_BCLR_ROWS; ++i) vn[i] = fr.hm[(size_t)(s_ry[jn][yb + i] + cx)];
#pragma unroll
			for (uint32_t i = 0; i < SMH_BCLR_ROWS; ++i) {
				const double z = clear_height(v[i], fr.zscale) - h0;
				const double x = d[i] * t, gxx = w.g * (x * x);
				const double m0 = bal_clear_sample(x, gxx, T[i][0], qq1[i][0], den, z), m1 = bal_clear_sample(x, gxx, T[i][1], qq1[i][1], den, z);
				blk[i][0] = blk[i][0] || m0 < r.margin_m;
				blk[i][1] = blk[i][1] || m1 < r.margin_m;
				los[i] = los[i] || bal_clear_los(alt[i], t, z);
				best[i] = m0 < best[i] ? m0 : best[i];
				v[i] = vn[i];
			}
		}
	}

	// ---- the bytes, the margin, the paint, the counts
	uint32_t packed = 0u;                                          // the lane's bytes inside the window, row i in byte i
#pragma unroll
	for (uint32_t i = 0; i < SMH_BCLR_ROWS; ++i) {
		const uint32_t Y = py0 + yb + i;
		const bool in = in_x && Y < r.out_h, none = d[i] == 0.0;
		uint32_t c = 0u, own = 0u;
		if (fl[i] & BCLR_F_VERDICT) {
			const bool oor = (fl[i] & BCLR_F_OOR) != 0u;
			own = bal_clear_class(oor, none, fl[i] & BCLR_F_UNUS0, blk[i][0]);
			c = own | (bal_clear_class(oor, none, fl[i] & BCLR_F_UNUS1, blk[i][1]) << 3);
			if (!none && los[i]) c |= SMHV_BCLR_LOS;
		}
		if (in) {
			const size_t at = (size_t)Y * r.out_w + X;
			packed |= c << (8u * i);
			if (PLANES) {
				if (bytes_out) bytes_out[at] = (uint8_t)c;
				if (margin_out) margin_out[at] = own >= SMHV_BCLR_CLEAR ? (float)((none || S == 1u) ? 0.0 : bal_clear_margin(best[i])) : __builtin_nanf("");
			}
			if (PAINT && c) {
				uint32_t *p = (uint32_t *)(r.img + (size_t)f * r.img_stride) + at;
				uint32_t px = reach_blend(*p, s_pal[own - 1u]);
				if ((own == SMHV_BCLR_UNUSABLE || own == SMHV_BCLR_BLOCKED) && (c >> 3 & 7u) == SMHV_BCLR_CLEAR) px = reach_blend(px, s_pal[4]);
				if (c & SMHV_BCLR_LOS) px = reach_blend(px, s_pal[5]);
				*p = px;
			}
		}
	}
#pragma unroll
	for (uint32_t k = 0; k < BCLR_CNT; ++k) {
		uint32_t cnt = 0u;
#pragma unroll
		for (uint32_t i = 0; i < SMH_BCLR_ROWS; ++i) {
			const uint32_t c = (packed >> (8u * i)) & 255u, own = c & 7u, oth = (c >> 3) & 7u;
			const bool hit = k < 4u ? own == k + 1u : k < 8u ? oth == k - 3u : k == 8u ? (c & SMHV_BCLR_LOS) != 0u
			                 : (own == SMHV_BCLR_UNUSABLE || own == SMHV_BCLR_BLOCKED) && oth == SMHV_BCLR_CLEAR;
			cnt += (uint32_t)__popcll(__ballot(hit));
		}
		if (lane == 0u && cnt) atomicAdd(&s_cnt[k], cnt);
	}
	__syncthreads();
	smhv_ballistic_clearance_map_result *out = &r.out[f];
	if (tid < 4u) { if (s_cnt[tid]) atomicAdd(&out->own[tid], s_cnt[tid]); }
	else if (tid < 8u) { if (s_cnt[tid]) atomicAdd(&out->other[tid - 4u], s_cnt[tid]); }
	else if (tid == 8u) { if (s_cnt[8]) atomicAdd(&out->los_blocked, s_cnt[8]); }
	else if (tid == 9u) { if (s_cnt[9]) atomicAdd(&out->switch_arc, s_cnt[9]); }
	else if (tid == 10u && blockIdx.x == 0u && blockIdx.y == 0u) { out->valid = 1u; out->origin[0] = ox; out->origin[1] = oy; }
}

hipError_t launch_bclear_lines(const BalClearLinesRun &r, uint32_t n, hipStream_t s) {
	const uint32_t lines = r.per_call ? r.n_lines : (uint32_t)SMHV_MAX_LINES;
	if (n == 0u || n > 65535u || lines == 0u || r.samples == 0u || r.samples > SMHV_CLEAR_MAX_SAMPLES ||
	    (r.per_call ? (n != 1u || !r.lines || !r.out_lines) : (!r.res || !r.out)))
		return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_bclear_lines, dim3(lines, n), dim3(128), 0, s, r);
	return hipGetLastError();
}

hipError_t launch_bclear_map(const BalClearMapRun &r, uint32_t n, bool paint, hipStream_t s) {
	if (n == 0u || n > 65535u || r.out_w == 0u || r.out_h == 0u || !r.out || (paint && !r.img) || (!r.per_call && (!r.aux || !r.res)) ||
	    r.samples == 0u || r.samples > SMHV_CLEAR_MAX_SAMPLES)
		return hipErrorInvalidValue;
	const bool planes = r.bytes || r.margin;
	const dim3 grid((r.out_w + SMH_REACH_TW - 1u) / SMH_REACH_TW, (r.out_h + SMH_REACH_TH - 1u) / SMH_REACH_TH, n), block(SMH_BCLR_THREADS);
	if (paint && planes) hipLaunchKernelGGL((k_bclear_map<true, true>), grid, block, 0, s, r);
	else if (paint) hipLaunchKernelGGL((k_bclear_map<true, false>), grid, block, 0, s, r);
	else if (planes) hipLaunchKernelGGL((k_bclear_map<false, true>), grid, block, 0, s, r);
	else hipLaunchKernelGGL((k_bclear_map<false, false>), grid, block, 0, s, r);
	return hipGetLastError();
}

}  // namespace smh
