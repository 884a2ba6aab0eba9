// smh_clear.hip -- terrain clearance: the heightmap sampled along a line of fire, held against the high-angle arc and the straight
// sight line (include/smh_vision_hip.h, "terrain clearance": the semantics are pinned there; the steps of the rule are smh_firing.h's
// clear_coord / clear_texel / clear_arc / clear_sample, shared by both kernels).
//
// k_clear_lines: one wave per (frame, line, direction), two waves per workgroup.  The end points go through firing_line()'s own
//   operations; the lanes stride the interior samples (k = 1 + lane, 65 + lane, ...), counts come from ballots, min_margin / min_at
//   and first_blocked from a butterfly of shuffles whose order is total ((m, k) with distinct k), so every lane ends with the
//   sequential rule's answer.  Lane 0 writes the record; the lanes of direction 0 write the profile.
// k_clear_map<PAINT, BYTES>: k_reach's tiles (SMH_REACH_TW x SMH_REACH_TH, 256 threads, a lane owns one column and SMH_REACH_ROWS
//   rows).  Columns and rows are evaluated once per tile (reach_axis and the target's own coordinate).  A sample's texel is separable
//   -- its column depends on the pixel's column and k alone, its row on the pixel's row and k -- and so is t = k / S: the workgroup
//   stages them in LDS for SMH_CLEAR_KC samples at a time (one f64 division per sample and eight threads, not two per pixel and
//   sample), 80 entries per sample where the tile's pixels would evaluate 2048.  The march reads t and the column's texel once per
//   sample and serves the lane's four rows from them: four independent u16 gathers per lane and sample (neighbouring lanes hit
//   neighbouring texels of one heightmap row), asked for one sample ahead of their use, so they are in flight while the previous
//   sample's arithmetic runs.  What is left per pixel and sample is the rule's f64 arithmetic: the texel's height (v / 65535 in three
//   operations: smh_firing.h, clear_height) and the arc with its one true division (/ (2 V^2)).  Nobody leaves the march early: every lane
//   runs every sample, so no count can depend on a choice.  Staged coordinates are clamped into the heightmap, so a lane without a
//   verdict loads in bounds and drops what it computed.
//   Counts go k_reach's way: ballots, one LDS atomic per wave and count, one global vector atomic per workgroup and count.
// No scratch; every array below is indexed by unrolled constants or lies in LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smh_firing.h"

namespace smh {

#define CLR_NO_K 0xFFFFFFFFu   // min_at while no sample has replaced the starting +inf

__global__ void __launch_bounds__(128) k_clear_lines(const ClearLinesRun r) {
	const uint32_t l = blockIdx.x, f = blockIdx.y, lane = threadIdx.x & 63u, dir = threadIdx.x >> 6;
	const uint32_t S = r.samples;
	// ---- the line and where its results go
	bool live, has_mm;
	uint32_t mm[4];
	smhv_line ln = {0.0f, 0.0f, 0.0f, 0.0f};
	smhv_clearance_dir *out;
	float *prof = nullptr;
	if (r.per_call) {
		live = l < r.n_lines;
		if (!live) return;
		ln = r.lines[l];
		has_mm = r.has_mm != 0u;
		mm[0] = r.mm[0]; mm[1] = r.mm[1]; mm[2] = r.mm[2]; mm[3] = r.mm[3];
		out = &r.out_lines[l].dir[dir];
		if (r.profiles) prof = r.profiles + (size_t)l * SMH_CLEAR_PROFILE;
	} else {
		const smhv_frame_result *res = &r.res[f];
		const uint32_t n = res->n_lines;
		live = l < n;
		if (live) ln = res->lines[l];
		has_mm = res->has_minimap != 0u;
		mm[0] = res->minimap[0]; mm[1] = res->minimap[1]; mm[2] = res->minimap[2]; mm[3] = res->minimap[3];
		out = &r.out[f].line[l].dir[dir];
		if (r.profiles) prof = r.profiles + ((size_t)f * SMHV_MAX_LINES + l) * SMH_CLEAR_PROFILE;
		if (l == 0u && threadIdx.x == 0u) { r.out[f].n_lines = n; r.out[f].reserved = 0u; }
	}
	if (dir != 0u) prof = nullptr;

	// ---- the end points: firing_line()'s heightmap branch
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
		if (lane == 0u) *out = smhv_clearance_dir{0u, 0u, 0u, 0u, 0.0, 0u, 0u};
		if (prof)
			for (uint32_t k = lane; k < SMH_CLEAR_PROFILE; k += 64u) prof[k] = 0.0f;
		return;
	}
	const float e0 = (float)h0, e1 = (float)h1;                     // the profile's ends (direction 0)
	double alt = h1 - h0;
	if (dir != 0u) {                                               // the line (P1, P0)
		double s;
		s = x0; x0 = x1; x1 = s;
		s = y0; y0 = y1; y1 = s;
		h0 = h1;
		alt = -alt;
	}
	const ClearArc arc = clear_arc(d, alt);
	const bool oor = !(arc.disc >= 0.0), none = d == 0.0;          // no arc / no samples

	// ---- the interior samples, 64 at a time
	uint32_t n_blocked = 0u, n_los = 0u, first = S, at = CLR_NO_K;
	double best = __builtin_inf();
	for (uint32_t base = 1u; base < S; base += 64u) {
		const uint32_t k = base + lane;
		const bool act = k < S && !none;
		const double t = (double)k / (double)S;
		const uint32_t sx = clear_texel(x0, x1, t, fr.hm_w), sy = clear_texel(y0, y1, t, fr.hm_h);
		const double hgt = clear_height(fr.hm[(size_t)sy * fr.hm_w + (size_t)sx], fr.zscale);   // (clamped: in bounds for every lane)
		bool los;
		const double m = clear_sample(arc, t, hgt - h0, &los);
		const bool blk = act && !oor && m < r.margin_m;
		n_blocked += (uint32_t)__popcll(__ballot(blk));
		n_los += (uint32_t)__popcll(__ballot(act && los));
		if (blk) first = min(first, k);
		if (act && !oor && m < best) { best = m; at = k; }
		if (prof && k < S) prof[k] = (float)hgt;
	}
#pragma unroll
	for (int off = 32; off; off >>= 1) {
		const double ob = __shfl_xor(best, off);
		const uint32_t oa = __shfl_xor(at, off);
		if (ob < best || (ob == best && oa < at)) { best = ob; at = oa; }
		first = min(first, (uint32_t)__shfl_xor(first, off));
	}
	if (lane == 0u) {
		smhv_clearance_dir o;
		o.status = oor ? SMHV_CLEAR_OUT_OF_RANGE : n_blocked ? SMHV_CLEAR_BLOCKED : SMHV_CLEAR_CLEAR;
		o.first_blocked = first;
		o.n_blocked = n_blocked;
		o.los_blocked = n_los;
		o.min_margin = (oor || none || S == 1u) ? 0.0 : best;
		o.min_at = at == CLR_NO_K ? 0u : at;
		o.reserved = 0u;
		*out = o;
	}
	if (prof)
		for (uint32_t k = lane; k < SMH_CLEAR_PROFILE; k += 64u) {
			if (k == 0u) prof[k] = e0;
			else if (k == S) prof[k] = e1;
			else if (k > S) prof[k] = 0.0f;
		}
}

// the heightmap coordinate of a window pixel's target on one axis (c = the pixel's centre), and of the origin: reach_axis()'s c1, c0
__device__ __forceinline__ double clear_target_coord(float c, float s, float t, float r0, double rlen, uint32_t n) {
	const float tg = (c - t) / s;                                  // MapViewport::inverse_xy
	const float p1 = tg * s + t;                                   // MapViewport::translate_xy
	return clear_coord(p1, r0, rlen, n);
}
__device__ __forceinline__ double clear_origin_coord(float o, float s, float t, float r0, double rlen, uint32_t n) {
	const float p0 = o * s + t;
	return clear_coord(p0, r0, rlen, n);
}

template <bool PAINT, bool BYTES>
__global__ void __launch_bounds__(256) k_clear_map(const ClearMapRun r) {
	__shared__ ReachAxis s_col[SMH_REACH_TW], s_row[SMH_REACH_TH];
	__shared__ double s_c1x[SMH_REACH_TW], s_c1y[SMH_REACH_TH];    // the targets' own heightmap coordinates
	__shared__ double s_org[3];                                    // the origin's heightmap coordinates and its height
	__shared__ double s_t[SMH_CLEAR_KC];                           // the staged samples: t ...
	__shared__ uint32_t s_cx[SMH_CLEAR_KC][SMH_REACH_TW];          //   ... the texel column of each tile column ...
	__shared__ uint32_t s_ry[SMH_CLEAR_KC][SMH_REACH_TH];          //   ... and the texel row of each tile row, times the heightmap's width
	__shared__ uint32_t s_cnt[4], s_pal[4];                        // statuses 1 .. 3 and the LOS pixels; the palette
	const uint32_t f = blockIdx.z, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const uint32_t px0 = blockIdx.x * SMH_REACH_TW, py0 = blockIdx.y * SMH_REACH_TH;
	const uint32_t X = px0 + lane, yb = wave * SMH_REACH_ROWS;
	const bool in_x = X < r.out_w;
	uint8_t *bytes_out = BYTES ? r.bytes + (size_t)f * r.bytes_stride : nullptr;

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
		if (BYTES && in_x) {
#pragma unroll
			for (uint32_t i = 0; i < SMH_REACH_ROWS; ++i) {
				const uint32_t Y = py0 + yb + i;
				if (Y < r.out_h) bytes_out[(size_t)Y * r.out_w + X] = 0u;
			}
		}
		return;
	}

	// ---- the tile's columns and rows, the origin
	const FiringRun &fr = r.fr;
	const bool use_hm = has_mm && fr.hm != nullptr;
	HmRect q = {0.0f, 0.0f, 0.0f, 0.0f};
	double rw = 0.0, rh = 0.0;
	if (use_hm) {
		q = hm_rect(mm, fr.flags, fr.b0x, fr.b0y, fr.hm_w, fr.hm_h, fr.sw, fr.sh, fr.tx, fr.ty);
		rw = (double)(q.r - q.l); rh = (double)(q.b - q.t);
	}
	if (tid < 4u) s_cnt[tid] = 0u;
	else if (tid < 8u) s_pal[tid - 4u] = r.pal[tid - 4u];
	if (tid >= 64u && tid < 64u + SMH_REACH_TW) {
		const uint32_t e = tid - 64u;
		const float c = (float)(px0 + e) + 0.5f;
		s_col[e] = reach_axis(c, ox, fr.sw, fr.tx, use_hm, q.l, rw, fr.hm_w);
		s_c1x[e] = use_hm ? clear_target_coord(c, fr.sw, fr.tx, q.l, rw, fr.hm_w) : 0.0;
	} else if (tid >= 128u && tid < 128u + SMH_REACH_TH) {
		const uint32_t e = tid - 128u;
		const float c = (float)(py0 + e) + 0.5f;
		s_row[e] = reach_axis(c, oy, fr.sh, fr.ty, use_hm, q.t, rh, fr.hm_h);
		s_c1y[e] = use_hm ? clear_target_coord(c, fr.sh, fr.ty, q.t, rh, fr.hm_h) : 0.0;
	} else if (tid == 192u) {
		double c0x = 0.0, c0y = 0.0, h0 = 0.0;
		if (use_hm) {
			c0x = clear_origin_coord(ox, fr.sw, fr.tx, q.l, rw, fr.hm_w); c0y = clear_origin_coord(oy, fr.sh, fr.ty, q.t, rh, fr.hm_h);
			const int32_t ix0 = reach_origin_texel(ox, fr.sw, fr.tx, q.l, rw, fr.hm_w), iy0 = reach_origin_texel(oy, fr.sh, fr.ty, q.t, rh, fr.hm_h);
			if (ix0 >= 0 && iy0 >= 0) h0 = clear_height(fr.hm[(size_t)iy0 * fr.hm_w + (size_t)ix0], fr.zscale);
		}
		s_org[0] = c0x; s_org[1] = c0y; s_org[2] = h0;
	}
	__syncthreads();

	// ---- the lane's pixels: the verdict's inputs (the rule's steps 1 and 2)
	const ReachAxis col = s_col[lane];
	const double c0x = s_org[0], c0y = s_org[1], h0 = s_org[2];
	ClearArc arc[SMH_REACH_ROWS];
	bool verdict[SMH_REACH_ROWS], blk[SMH_REACH_ROWS], los[SMH_REACH_ROWS];
#pragma unroll
	for (uint32_t i = 0; i < SMH_REACH_ROWS; ++i) {
		const ReachAxis row = s_row[yb + i];
		verdict[i] = col.ix >= 0 && row.ix >= 0;                    // the heightmap branch: the origin and the target inside
		const uint16_t v = verdict[i] ? fr.hm[(size_t)row.ix * fr.hm_w + (size_t)col.ix] : (uint16_t)0u;
		const double dx = col.dh, dy = row.dh;
		arc[i] = clear_arc(sqrt(dx * dx + dy * dy), clear_height(v, fr.zscale) - h0);
		blk[i] = false; los[i] = false;
	}

	// ---- the march: SMH_CLEAR_KC samples staged, then walked by every lane
	const uint32_t S = r.samples, n_int = use_hm ? S - 1u : 0u;       // interior samples (none without a heightmap: no verdict anywhere)
	for (uint32_t base = 0; base < n_int; base += SMH_CLEAR_KC) {
		if (base) __syncthreads();                                 // (the previous samples have been read)
		{
			const uint32_t j = tid >> 3, part = tid & 7u;             // eight threads per sample
			const double t = (double)(1u + base + j) / (double)S;
			if (part == 0u) s_t[j] = t;
			for (uint32_t e = part; e < SMH_REACH_TW + SMH_REACH_TH; e += 8u) {
				if (e < SMH_REACH_TW) s_cx[j][e] = clear_texel(c0x, s_c1x[e], t, fr.hm_w);
				else s_ry[j][e - SMH_REACH_TW] = clear_texel(c0y, s_c1y[e - SMH_REACH_TW], t, fr.hm_h) * fr.hm_w;
			}
		}
		__syncthreads();
		const uint32_t nk = min(SMH_CLEAR_KC, n_int - base);
		// the texels of sample j + 1 are on their way while sample j is held against the arc (the last sample asks for its own again)
		uint16_t v[SMH_REACH_ROWS];
#pragma unroll
		for (uint32_t i = 0; i < SMH_REACH_ROWS; ++i) v[i] = fr.hm[(size_t)(s_ry[0][yb + i] + s_cx[0][lane])];   // (w * h <= 2^28; clamped: in bounds for every lane)
#pragma unroll 2
		for (uint32_t j = 0; j < nk; ++j) {
			const double t = s_t[j];
			const uint32_t jn = min(j + 1u, nk - 1u), cx = s_cx[jn][lane];
			uint16_t vn[SMH_REACH_ROWS];
#pragma unroll
			for (uint32_t i = 0; i < SMH_REACH_ROWS; ++i) vn[i] = fr.hm[(size_t)(s_ry[jn][yb + i] + cx)];
#pragma unroll
			for (uint32_t i = 0; i < SMH_REACH_ROWS; ++i) {
				bool l;
				const double m = clear_sample(arc[i], t, clear_height(v[i], fr.zscale) - h0, &l);
				blk[i] = blk[i] || m < r.margin_m;
				los[i] = los[i] || l;
				v[i] = vn[i];
			}
		}
	}

	// ---- the bytes, the paint, the counts
	uint32_t packed = 0u;                                          // the lane's bytes inside the window, row i in byte i
#pragma unroll
	for (uint32_t i = 0; i < SMH_REACH_ROWS; ++i) {
		const uint32_t Y = py0 + yb + i;
		const bool in = in_x && Y < r.out_h, live = verdict[i] && arc[i].d != 0.0;
		uint32_t c = 0u;
		if (verdict[i]) {
			c = !(arc[i].disc >= 0.0) ? SMHV_CLEAR_OUT_OF_RANGE : (live && blk[i]) ? SMHV_CLEAR_BLOCKED : SMHV_CLEAR_CLEAR;
			if (live && los[i]) c |= SMHV_CLEAR_LOS_BLOCKED;
		}
		if (in) packed |= c << (8u * i);
		if (BYTES && in) bytes_out[(size_t)Y * r.out_w + X] = (uint8_t)c;
		if (PAINT && in && c) {
			uint32_t *p = (uint32_t *)(r.img + (size_t)f * r.img_stride) + (size_t)Y * r.out_w + X;
			uint32_t px = reach_blend(*p, s_pal[(c & 0x7Fu) - 1u]);
			if (c & SMHV_CLEAR_LOS_BLOCKED) px = reach_blend(px, s_pal[3]);
			*p = px;
		}
	}
#pragma unroll
	for (uint32_t k = 0; k < 4u; ++k) {
		uint32_t cnt = 0u;
#pragma unroll
		for (uint32_t i = 0; i < SMH_REACH_ROWS; ++i) {
			const uint32_t c = (packed >> (8u * i)) & 255u;
			cnt += (uint32_t)__popcll(__ballot(k < 3u ? (c & 0x7Fu) == k + 1u : (c & SMHV_CLEAR_LOS_BLOCKED) != 0u));
		}
		if (lane == 0u && cnt) atomicAdd(&s_cnt[k], cnt);
	}
	__syncthreads();
	smhv_clearance_map_result *out = &r.out[f];
	if (tid < 3u) { if (s_cnt[tid]) atomicAdd(&out->count[tid], s_cnt[tid]); }
	else if (tid == 3u) { if (s_cnt[3]) atomicAdd(&out->los_blocked, s_cnt[3]); }
	else if (tid == 4u && blockIdx.x == 0u && blockIdx.y == 0u) { out->valid = 1u; out->origin[0] = ox; out->origin[1] = oy; }
}

hipError_t launch_clear_lines(const ClearLinesRun &r, uint32_t n, hipStream_t s) {
	const uint32_t lines = r.per_call ? r.n_lines : (uint32_t)SMHV_MAX_LINES;
	if (n == 0u || n > 65535u || lines == 0u || r.samples == 0u || r.samples > SMHV_CLEAR_MAX_SAMPLES ||
	    (r.per_call ? (n != 1u || !r.lines || !r.out_lines) : (!r.res || !r.out)))
		return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_clear_lines, dim3(lines, n), dim3(128), 0, s, r);
	return hipGetLastError();
}

hipError_t launch_clear_map(const ClearMapRun &r, uint32_t n, bool paint, bool bytes, hipStream_t s) {
	if (n == 0u || n > 65535u || r.out_w == 0u || r.out_h == 0u || !r.out || (paint && !r.img) || (bytes && !r.bytes) || (!r.per_call && (!r.aux || !r.res)) ||
	    r.samples == 0u || r.samples > SMHV_CLEAR_MAX_SAMPLES)
		return hipErrorInvalidValue;
	const dim3 grid((r.out_w + SMH_REACH_TW - 1u) / SMH_REACH_TW, (r.out_h + SMH_REACH_TH - 1u) / SMH_REACH_TH, n), block(256);
	if (paint && bytes) hipLaunchKernelGGL((k_clear_map<true, true>), grid, block, 0, s, r);
	else if (paint) hipLaunchKernelGGL((k_clear_map<true, false>), grid, block, 0, s, r);
	else if (bytes) hipLaunchKernelGGL((k_clear_map<false, true>), grid, block, 0, s, r);
	else hipLaunchKernelGGL((k_clear_map<false, false>), grid, block, 0, s, r);
	return hipGetLastError();
}

}  // namespace smh
