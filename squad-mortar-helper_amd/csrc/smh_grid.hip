// smh_grid.hip -- the map grid: the cell, the keypad digits, the grid line and the cell label of every pixel of a map view's window,
// drawn into the render slab, as a flag byte plane, a u32 cell plane and per-frame counts; and the grid references of the line ends
// (include/smh_vision_hip.h, "map grid": the semantics are pinned there; the rule is smh_grid.h's, the rectangle smh_firing.h's
// hm_rect, the blend its reach_blend).
//
// k_grid<PAINT, PLANES> over frames x tiles of SMH_REACH_TW x SMH_REACH_TH window pixels, 256 threads: k_reach's and k_relief's shape.
//   Frame-uniform inputs (open, the minimap rectangle, m/px) are read once per workgroup; a frame without a grid leaves at once (with
//   PLANES its tile's plane elements are zeroed first), paints nothing and counts nothing.
//   The mapping is separable, and so is everything that follows from it.  The TW + 1 columns and TH + 1 rows a tile and its +1
//   neighbours touch are evaluated once each, by one thread each, into LDS (GridEntry): idx_L by the axis' one f64 division, the
//   axis' share of "has a cell", its share of the cell word (the digit of a level is (cx + 1) + (2 - cy) * 3: a sum of a column's and
//   a row's part), with labels the cell's first column by grid_first and from it the glyph and the glyph's column or row of this
//   entry, and the characters the axis contributes.  Behind a barrier the same threads compare their entry with the next one: the
//   level at which a column and its right neighbour cross does not depend on the row.  No division and no search runs per pixel.
//   A lane owns one column and SMH_REACH_ROWS consecutive rows.  Per pixel: two LDS entries, an AND, a minimum, with labels one font
//   byte from LDS and a bit test, the plane stores, and on a line or label pixel a load, the blend and a store.
//   Counts: the lane's flag bytes are kept packed; after the rows, wave ballots and popcounts, one LDS atomic per wave and count, one
//   global vector atomic per workgroup and count that is not zero.  The first and last column and row: as keys whose identity is 0
//   (~v for a minimum, v + 1 or row1 for a maximum), one LDS and one global atomicMax each; k_grid_finish, one thread per frame
//   behind k_grid on the stream, turns the keys into the numbers.
// k_grid_refs: one lane per line end through grid_ref_of; a batch frame is one wave (SMHV_MAX_LINES lines, two ends each).
// No scratch; every array below is indexed by unrolled constants or lies in LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smh_firing.h"
#include "smh_font5x7_ascii.h"
#include "smh_grid.h"

namespace smh {

__constant__ uint8_t c_grid_font[SMH_TEXT_FONT_GLYPHS][SMH_TEXT_FONT_ROWS] = SMH_FONT5X7_ASCII_TABLE;
#define SMH_GRID_FONT_FIRST 16u          // '0' - 0x20: the labels are made of '0' .. '9' and 'A' .. 'Z'
#define SMH_GRID_FONT_BYTES ((0x5Au - 0x30u + 1u) * SMH_TEXT_FONT_ROWS)
#define SMH_GRID_LAB_NONE 0xFFFFu

struct GridEntry {
	int32_t idx;                         // idx_L
	uint32_t ok;                         // the axis' share of "has a cell"
	uint32_t word;                       // ... of the cell word
	uint32_t lvl;                        // the level at which this entry and the next cross (4: none; needs both ok)
	uint32_t lab;                        // a column: glyph | glyph column << 8; a row: the glyph row; SMH_GRID_LAB_NONE: no label passes here
	uint32_t chars;                      // a column: the letters; a row: the digits | their number << 24 (a column's number: bit 24 .. 25 too)
};

// The two axes of a frame, its source and what is drawn
struct GridFrame { GridAxis x, y; uint32_t source; int32_t Ld; uint32_t labels; };
__device__ __forceinline__ GridFrame grid_frame(const GridRun &r, bool have, const uint32_t mm[4], bool has_mpx, double mpx) {
	GridFrame g;
	const bool use_hm = r.fr.hm != nullptr;
	g.source = !have ? SMHV_GRID_NONE : use_hm ? SMHV_GRID_HEIGHTMAP : has_mpx ? SMHV_GRID_SCALES : SMHV_GRID_NONE;
	const HmRect q = hm_rect(mm, use_hm ? r.fr.flags : 0u, r.fr.b0x, r.fr.b0y, r.fr.hm_w, r.fr.hm_h, r.fr.sw, r.fr.sh, r.fr.tx, r.fr.ty);
	if (use_hm) {
		g.x = grid_axis_heightmap(q.l, q.r, r.fr.hm_w, r.origin_m[0], r.cell_m, r.levels);
		g.y = grid_axis_heightmap(q.t, q.b, r.fr.hm_h, r.origin_m[1], r.cell_m, r.levels);
	} else {
		g.x = grid_axis_scales(q.l, q.r, r.fr.sw, mpx, r.origin_m[0], r.cell_m, r.levels);
		g.y = grid_axis_scales(q.t, q.b, r.fr.sh, mpx, r.origin_m[1], r.cell_m, r.levels);
	}
	g.Ld = grid_drawn_levels(r.cell_m, r.levels, g.x.ppm, g.y.ppm, r.min_px);
	g.labels = grid_labels_drawn(r.cell_m, g.x, g.y, g.Ld, r.pal[4] >> 24, r.label_min_px) ? 1u : 0u;
	return g;
}

// the entry of integer column (or row) P of axis a; `row`: the y axis
__device__ __forceinline__ GridEntry grid_entry(const GridAxis &a, int32_t P, bool row, bool labels) {
	GridEntry e;
	const GridIdx i = grid_index(a, (float)P + 0.5f);
	const uint32_t L = a.L;
	e.idx = i.idx;
	e.ok = grid_axis_cell(a, i, row ? SMHV_GRID_MAX_ROWS : SMHV_GRID_MAX_COLS) ? 1u : 0u;
	e.word = 0u; e.lvl = 4u; e.lab = SMH_GRID_LAB_NONE; e.chars = 0u;
	if (e.ok) {
		const int32_t i0 = grid_level(i.idx, L, 0u);
		uint32_t w = row ? (uint32_t)(i0 + 1) << 10 : (uint32_t)i0;
#pragma unroll
		for (uint32_t k = 1u; k <= 3u; ++k)
			if (k <= L) {
				const uint32_t m = grid_mod3(grid_level(i.idx, L, k));
				w |= (row ? (2u - m) * 3u : m + 1u) << (16u + 4u * k);
			}
		e.word = w;
		if (labels) {
			const int32_t o = P - grid_first(a, P, i0) - 3;
			uint32_t n;
			if (row) {
				if (o >= 0 && o < (int32_t)SMH_TEXT_FONT_ROWS) e.lab = (uint32_t)o;
				e.chars = grid_row_digits((uint32_t)(i0 + 1), &n);
			} else {
				if (o >= 0 && o < 30 && o % 6 < 5) e.lab = (uint32_t)(o / 6) | (uint32_t)(o % 6) << 8;
				e.chars = grid_letters((uint32_t)i0, &n);
			}
			e.chars |= n << 24;
		}
	}
	return e;
}

template <bool PAINT, bool PLANES>
__global__ void __launch_bounds__(256) k_grid(const GridRun r) {
	__shared__ GridEntry s_col[SMH_REACH_TW + 1u], s_row[SMH_REACH_TH + 1u];
	__shared__ uint32_t s_cnt[6], s_ext[4];
	__shared__ uint8_t s_font[SMH_GRID_FONT_BYTES + 3u];
	const uint32_t f = blockIdx.z, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const uint32_t x0 = blockIdx.x * SMH_REACH_TW, y0 = blockIdx.y * SMH_REACH_TH;
	const uint32_t X = x0 + lane, yb = wave * SMH_REACH_ROWS;
	const bool in_x = X < r.out_w;
	uint8_t *bytes_out = PLANES && r.bytes ? r.bytes + (size_t)f * r.plane_stride : nullptr;
	uint32_t *cells_out = PLANES && r.cells ? r.cells + (size_t)f * r.plane_stride : nullptr;

	// ---- the frame: its minimap rectangle and its metres per pixel, or none
	bool have = r.has_mm != 0u, has_mpx = r.has_mpx != 0u;
	double mpx = r.mpx;
	uint32_t mm[4] = {r.mm[0], r.mm[1], r.mm[2], r.mm[3]};
	if (!r.per_call) {
		const smhv_frame_result *res = &r.res[f];
		have = r.aux[f].open != 0u && res->has_minimap != 0u;
		has_mpx = res->has_mpx != 0u; mpx = res->mpx;
		mm[0] = res->minimap[0]; mm[1] = res->minimap[1]; mm[2] = res->minimap[2]; mm[3] = res->minimap[3];
	}
	const GridFrame g = grid_frame(r, have, mm, has_mpx, mpx);
	if (g.source == SMHV_GRID_NONE) {                              // (uniform over the workgroup)
		if (PLANES && in_x) {
#pragma unroll
			for (uint32_t i = 0; i < SMH_REACH_ROWS; ++i) {
				const uint32_t Y = y0 + yb + i;
				if (Y < r.out_h) {
					const size_t at = (size_t)Y * r.out_w + X;
					if (bytes_out) bytes_out[at] = 0u;
					if (cells_out) cells_out[at] = 0u;
				}
			}
		}
		return;
	}

	// ---- the tile's columns and rows, then what each shares with the next
	const bool labels = g.labels != 0u;
	if (tid < 6u) s_cnt[tid] = 0u;
	else if (tid < 10u) s_ext[tid - 6u] = 0u;
	if (labels)
		for (uint32_t i = tid; i < SMH_GRID_FONT_BYTES; i += 256u) s_font[i] = ((const uint8_t *)c_grid_font)[SMH_GRID_FONT_FIRST * SMH_TEXT_FONT_ROWS + i];
	if (tid <= SMH_REACH_TW) s_col[tid] = grid_entry(g.x, (int32_t)(x0 + tid), false, labels);
	else if (tid >= 128u && tid <= 128u + SMH_REACH_TH) s_row[tid - 128u] = grid_entry(g.y, (int32_t)(y0 + tid - 128u), true, labels);
	__syncthreads();
	if (tid < SMH_REACH_TW) {
		const GridEntry a = s_col[tid], b = s_col[tid + 1u];
		if (a.ok & b.ok) s_col[tid].lvl = grid_cross(a.idx, b.idx, r.levels, g.Ld);
	} else if (tid >= 128u && tid < 128u + SMH_REACH_TH) {
		const GridEntry a = s_row[tid - 128u], b = s_row[tid - 127u];
		if (a.ok & b.ok) s_row[tid - 128u].lvl = grid_cross(a.idx, b.idx, r.levels, g.Ld);
	}
	__syncthreads();

	// ---- the lane's pixels, top to bottom
	const GridEntry col = s_col[lane];
	const uint32_t col_n = col.chars >> 24, gi = col.lab & 255u, gc = col.lab >> 8;
	uint32_t packed = 0u;                                          // the lane's flag bytes inside the window, row i in byte i
	uint32_t row_lo = 0u, row_hi = 0u;                             // the wave's keys of the first and last row1 (uniform)
#pragma unroll
	for (uint32_t i = 0; i < SMH_REACH_ROWS; ++i) {
		const uint32_t Y = y0 + yb + i;
		const GridEntry row = s_row[yb + i];
		const bool in = in_x && Y < r.out_h, has = (col.ok & row.ok) != 0u;
		const uint32_t lvl = has ? min(col.lvl, row.lvl) : 4u;
		bool lit = false;
		if (labels && has && col.lab != SMH_GRID_LAB_NONE && row.lab != SMH_GRID_LAB_NONE && gi < col_n + (row.chars >> 24)) {
			const uint32_t ch = gi < col_n ? (col.chars >> (8u * gi)) & 255u : (row.chars >> (8u * (gi - col_n))) & 255u;
			lit = ((s_font[(ch - 0x30u) * SMH_TEXT_FONT_ROWS + row.lab] >> (4u - gc)) & 1u) != 0u;
		}
		const uint32_t bits = has ? SMHV_GRID_HAS_CELL | (lvl < 4u ? (lvl + 1u) << 1 : 0u) | (lit ? SMHV_GRID_LABEL : 0u) : 0u;
		if (in) {
			const size_t at = (size_t)Y * r.out_w + X;
			packed |= bits << (8u * i);
			if (PLANES) {
				if (bytes_out) bytes_out[at] = (uint8_t)bits;
				if (cells_out) cells_out[at] = has ? col.word + row.word : 0u;
			}
			if (PAINT && (lvl < 4u || lit)) {
				uint32_t *p = (uint32_t *)(r.img + (size_t)f * r.img_stride) + at;
				uint32_t px = *p;
				if (lvl < 4u) px = reach_blend(px, lvl == 0u ? r.pal[0] : lvl == 1u ? r.pal[1] : lvl == 2u ? r.pal[2] : r.pal[3]);
				if (lit) px = reach_blend(px, r.pal[4]);
				*p = px;
			}
		}
		if (__ballot(in && has)) {                                    // (uniform: some pixel of this row of the wave has a cell)
			const uint32_t row1 = (row.word >> 10) & 1023u;
			row_lo = max(row_lo, ~row1);
			row_hi = max(row_hi, row1);
		}
	}

	// ---- the counts and the first and last column and row: per wave into LDS, per workgroup into the slab (cleared ahead of the launch)
#pragma unroll
	for (uint32_t k = 0; k < 6u; ++k) {
		uint32_t cnt = 0u;
#pragma unroll
		for (uint32_t i = 0; i < SMH_REACH_ROWS; ++i) {
			const uint32_t b = (packed >> (8u * i)) & 255u;
			const bool hit = k == 0u ? (b & SMHV_GRID_HAS_CELL) != 0u : k == 5u ? (b & SMHV_GRID_LABEL) != 0u : ((b >> 1) & 7u) == k;
			cnt += (uint32_t)__popcll(__ballot(hit));
		}
		if (lane == 0u && cnt) atomicAdd(&s_cnt[k], cnt);
	}
	const bool any = (packed & 0x01010101u) != 0u;
	uint32_t col_lo = any ? ~(col.word & 1023u) : 0u, col_hi = any ? (col.word & 1023u) + 1u : 0u;
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		col_lo = max(col_lo, (uint32_t)__shfl_xor((int)col_lo, d));
		col_hi = max(col_hi, (uint32_t)__shfl_xor((int)col_hi, d));
	}
	if (lane == 0u && col_hi) {                                    // (some pixel of the wave has a cell)
		atomicMax(&s_ext[0], col_lo);
		atomicMax(&s_ext[1], col_hi);
		atomicMax(&s_ext[2], row_lo);
		atomicMax(&s_ext[3], row_hi);
	}
	__syncthreads();
	smhv_grid_result *out = &r.out[f];
	if (tid == 0u) { if (s_cnt[0]) atomicAdd(&out->n_cell, s_cnt[0]); }
	else if (tid < 5u) { if (s_cnt[tid]) atomicAdd(&out->n_line[tid - 1u], s_cnt[tid]); }
	else if (tid == 5u) { if (s_cnt[5]) atomicAdd(&out->n_label, s_cnt[5]); }
	else if (tid == 6u) { if (s_ext[0]) atomicMax(&out->col_first, s_ext[0]); }
	else if (tid == 7u) { if (s_ext[1]) atomicMax(&out->col_last, s_ext[1]); }
	else if (tid == 8u) { if (s_ext[2]) atomicMax(&out->row_first, s_ext[2]); }
	else if (tid == 9u) { if (s_ext[3]) atomicMax(&out->row_last, s_ext[3]); }
	else if (blockIdx.x == 0u && blockIdx.y == 0u) {
		if (tid == 10u) out->valid = 1u;
		else if (tid == 11u) out->source = g.source;
		else if (tid == 12u) out->drawn_levels = (uint32_t)(g.Ld + 1);
	}
}

// the keys of n summaries into the first and last column and row (a frame without a cell keeps its zeros)
__global__ void __launch_bounds__(64) k_grid_finish(smhv_grid_result *out, uint32_t n) {
	const uint32_t f = blockIdx.x * 64u + threadIdx.x;
	if (f >= n || out[f].n_cell == 0u) return;
	out[f].col_first = ~out[f].col_first;
	out[f].col_last -= 1u;
	out[f].row_first = ~out[f].row_first;
}

// The references of the line ends.  Batch (r.refs): frame blockIdx.x, lane l = end l & 1 of line l >> 1, the whole record written.
// Per call (r.refs_out): end e = blockIdx.x * 64 + lane of r.lines.
__global__ void __launch_bounds__(64) k_grid_refs(const GridRun r) {
	const uint32_t lane = threadIdx.x;
	bool have = r.has_mm != 0u, has_mpx = r.has_mpx != 0u;
	double mpx = r.mpx;
	uint32_t mm[4] = {r.mm[0], r.mm[1], r.mm[2], r.mm[3]};
	uint32_t n_lines = r.n_lines, e = blockIdx.x * 64u + lane;
	const smhv_line *lines = r.lines;
	if (!r.per_call) {
		const smhv_frame_result *res = &r.res[blockIdx.x];
		have = r.aux[blockIdx.x].open != 0u && res->has_minimap != 0u;
		has_mpx = res->has_mpx != 0u; mpx = res->mpx;
		mm[0] = res->minimap[0]; mm[1] = res->minimap[1]; mm[2] = res->minimap[2]; mm[3] = res->minimap[3];
		n_lines = min(res->n_lines, (uint32_t)SMHV_MAX_LINES);
		lines = res->lines;
		e = lane;
	}
	const GridFrame g = grid_frame(r, have, mm, has_mpx, mpx);
	GridRefWords o;
	o.w[0] = 0u; o.w[1] = 0u; o.w[2] = 0u; o.w[3] = 0u; o.w[4] = 0u; o.w[5] = 0u;
	const bool live = e < 2u * n_lines;
	if (live && g.source != SMHV_GRID_NONE) {
		const smhv_line *ln = &lines[e >> 1];
		const float x = (e & 1u) ? ln->x1 : ln->x0, y = (e & 1u) ? ln->y1 : ln->y0;
		o = grid_ref_words(g.x, g.y, x * r.fr.sw + r.fr.tx, y * r.fr.sh + r.fr.ty);   // MapViewport::translate_xy
	}
	if (r.per_call) {
		if (live) *(GridRefWords *)&r.refs_out[e] = o;
		return;
	}
	smhv_grid_refs_result *out = &r.refs[blockIdx.x];
	*(GridRefWords *)&out->ref[lane >> 1][lane & 1u] = o;
	if (lane == 0u) { out->n_lines = n_lines; out->source = g.source; out->reserved[0] = 0u; out->reserved[1] = 0u; }
}
static_assert(SMHV_MAX_LINES == 32, "a frame's line ends are the lanes of one wave");

hipError_t launch_grid(const GridRun &r, uint32_t n, bool paint, hipStream_t s) {
	if (n == 0u || n > 65535u || r.out_w == 0u || r.out_h == 0u || !r.out || (paint && !r.img) || (!r.per_call && (!r.aux || !r.res)))
		return hipErrorInvalidValue;
	const bool planes = r.bytes || r.cells;
	const dim3 grid((r.out_w + SMH_REACH_TW - 1u) / SMH_REACH_TW, (r.out_h + SMH_REACH_TH - 1u) / SMH_REACH_TH, n), block(256);
	if (paint && planes) hipLaunchKernelGGL((k_grid<true, true>), grid, block, 0, s, r);
	else if (paint) hipLaunchKernelGGL((k_grid<true, false>), grid, block, 0, s, r);
	else if (planes) hipLaunchKernelGGL((k_grid<false, true>), grid, block, 0, s, r);
	else hipLaunchKernelGGL((k_grid<false, false>), grid, block, 0, s, r);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_grid_finish, dim3((n + 63u) / 64u), dim3(64), 0, s, r.out, n);
	return hipGetLastError();
}

hipError_t launch_grid_refs(const GridRun &r, uint32_t n, hipStream_t s) {
	if (r.per_call) {
		if (r.n_lines == 0u || !r.lines || !r.refs_out) return hipErrorInvalidValue;
		hipLaunchKernelGGL(k_grid_refs, dim3((2u * r.n_lines + 63u) / 64u), dim3(64), 0, s, r);
	} else {
		if (n == 0u || !r.refs || !r.aux || !r.res) return hipErrorInvalidValue;
		hipLaunchKernelGGL(k_grid_refs, dim3(n), dim3(64), 0, s, r);
	}
	return hipGetLastError();
}

}  // namespace smh
