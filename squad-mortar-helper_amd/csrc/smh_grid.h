// smh_grid.h -- the rule of the "map grid" (include/smh_vision_hip.h): metres of a window coordinate on one axis, its index at the
// finest level by one f64 division, every coarser index by integer floor division, cells, keypad digits, the text, the drawn levels,
// a cell's first column.  One text for the kernels (smh_grid.hip), the host helper (smh_grid.inc) and a stand-alone host check
// (tests/grid_rule_check.cpp compiles this header with the host compiler), hence SMH_HD.  Built with -ffp-contract=off: every f64
// operation below is the header's, in its order, unfused.  Below the rule, for the HIP build alone: the launch interface of
// smh_grid.hip (GridRun lives here and not in smh_kernels.h, which every other kernel file includes).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/smh_vision_hip.h"

#ifndef SMH_HD
#if defined(__HIPCC__)
#define SMH_HD __host__ __device__ __forceinline__
#else
#define SMH_HD static inline
#endif
#endif

namespace smh {

#define SMH_GRID_LABEL_SPAN 32           // columns to the left of a pixel that can decide its label: 5 glyphs of 6 columns and 3 more

// One axis of a frame.  m = (((double)c - (double)r0) / den) * mul: den = rlen and mul = (double)n on the heightmap branch, den =
// (double)s and mul = mpx on the scales branch; size = size_L; ppm = pixels per metre; rlen = (double)(r1 - r0).
struct GridAxis {
	double den, mul, origin, size, ppm, rlen;
	float r0, r1;
	uint32_t L, pad;
};
SMH_HD double grid_pow3(uint32_t k) { return k == 0u ? 1.0 : k == 1u ? 3.0 : k == 2u ? 9.0 : 27.0; }
SMH_HD GridAxis grid_axis_heightmap(float r0, float r1, uint32_t n, double origin, double cell_m, uint32_t L) {
	GridAxis a;
	a.r0 = r0; a.r1 = r1; a.rlen = (double)(r1 - r0);
	a.den = a.rlen; a.mul = (double)n; a.ppm = a.rlen / (double)n;
	a.origin = origin; a.size = cell_m / grid_pow3(L); a.L = L; a.pad = 0u;
	return a;
}
SMH_HD GridAxis grid_axis_scales(float r0, float r1, float s, double mpx, double origin, double cell_m, uint32_t L) {
	GridAxis a;
	a.r0 = r0; a.r1 = r1; a.rlen = (double)(r1 - r0);
	a.den = (double)s; a.mul = mpx; a.ppm = (double)s / mpx;
	a.origin = origin; a.size = cell_m / grid_pow3(L); a.L = L; a.pad = 0u;
	return a;
}

SMH_HD bool grid_finite(double v) { return v - v == 0.0; }           // (inf - inf and NaN - NaN are NaN)
// floor division by 3 and the non-negative remainder
SMH_HD int32_t grid_div3(int32_t v) { const int32_t q = v / 3; return v % 3 < 0 ? q - 1 : q; }
SMH_HD uint32_t grid_mod3(int32_t v) { const int32_t m = v % 3; return (uint32_t)(m < 0 ? m + 3 : m); }
// idx_k from idx_L
SMH_HD int32_t grid_level(int32_t idx, uint32_t L, uint32_t k) {
	for (uint32_t j = 3u; j > 0u; --j)
		if (j <= L && j > k) idx = grid_div3(idx);
	return idx;
}

// The entry of an f32 coordinate: g, IN, and idx_L (has: it exists; qf lies in [-2^31, 2^31), so the index is held in 32 bits)
struct GridIdx { double g; int32_t idx; uint32_t in, has, pad; };
SMH_HD GridIdx grid_index(const GridAxis &a, float c) {
	GridIdx e;
	const double m = (((double)c - (double)a.r0) / a.den) * a.mul;
	e.g = m - a.origin;
	const bool fin = grid_finite(e.g);
	e.in = (a.r0 <= c && c < a.r1 && fin) ? 1u : 0u;
	const double qf = floor(e.g / a.size);
	e.has = (fin && qf >= -2147483648.0 && qf < 2147483648.0) ? 1u : 0u;
	e.idx = e.has ? (int32_t)qf : 0;
	e.pad = 0u;
	return e;
}
// the axis' share of "has a cell": IN, an index, and idx_0 in [0, limit) -- limit = SMHV_GRID_MAX_COLS or SMHV_GRID_MAX_ROWS
SMH_HD bool grid_axis_cell(const GridAxis &a, const GridIdx &e, uint32_t limit) {
	if (!(e.in & e.has)) return false;
	const int32_t i0 = grid_level(e.idx, a.L, 0u);
	return i0 >= 0 && i0 < (int32_t)limit;
}
// the level at which two entries of one axis cross: the least k <= Ld at which their idx_k differ; 4: none
SMH_HD uint32_t grid_cross(int32_t ia, int32_t ib, uint32_t L, int32_t Ld) {
	uint32_t lvl = 4u;
	for (uint32_t j = 4u; j > 0u; --j) {                            // k = j - 1 = 3 .. 0
		const uint32_t k = j - 1u;
		if (k > L) continue;
		if (ia != ib && (int32_t)k <= Ld) lvl = k;
		ia = grid_div3(ia); ib = grid_div3(ib);
	}
	return lvl;
}
// Ld
SMH_HD int32_t grid_drawn_levels(double cell_m, uint32_t L, double ppm_x, double ppm_y, double min_px) {
	int32_t ld = -1;
	for (uint32_t k = 0u; k < 4u; ++k) {
		const double size = cell_m / grid_pow3(k);
		if (k <= L && size * ppm_x >= min_px && size * ppm_y >= min_px) ld = (int32_t)k;
	}
	return ld;
}
SMH_HD bool grid_labels_drawn(double cell_m, const GridAxis &x, const GridAxis &y, int32_t Ld, uint32_t label_weight, double label_min_px) {
	return Ld >= 0 && label_weight != 0u && x.rlen > 0.0 && y.rlen > 0.0 && cell_m * x.ppm >= label_min_px && cell_m * y.ppm >= label_min_px;
}

// Does the entry of integer column X have idx_0 == own0?
SMH_HD bool grid_column_is(const GridAxis &a, int32_t X, int32_t own0) {
	const GridIdx e = grid_index(a, (float)X + 0.5f);
	return e.has && grid_level(e.idx, a.L, 0u) == own0;
}
// Xfirst of a column X whose own idx_0 is own0, sought in [X - SMH_GRID_LABEL_SPAN, X]: the columns of one idx_0 are consecutive (every
// step of the rule is monotone in c), so an estimate from the inverse mapping is corrected by the forward rule -- downwards while the
// column before it still belongs to the cell, upwards while it does not belong itself.  The estimate decides only how many steps
// that takes.
SMH_HD int32_t grid_first(const GridAxis &a, int32_t X, int32_t own0) {
	const int32_t lo = X - SMH_GRID_LABEL_SPAN;
	const double cb = (((double)own0 * (a.size * grid_pow3(a.L)) + a.origin) / a.mul) * a.den + (double)a.r0;
	double e = ceil(cb - 0.5);
	if (!(e >= (double)lo)) e = (double)lo;
	if (e > (double)X) e = (double)X;
	int32_t x = (int32_t)e;
	if (grid_column_is(a, x, own0)) {
		while (x > lo && grid_column_is(a, x - 1, own0)) --x;
	} else {
		while (x < X && !grid_column_is(a, x, own0)) ++x;
	}
	return x;
}

// the column's letters and the row's digits, first character in the lowest byte; *n = how many
SMH_HD uint32_t grid_letters(uint32_t col, uint32_t *n) {
	if (col < 26u) { *n = 1u; return 65u + col; }
	const uint32_t c = col - 26u;
	*n = 2u;
	return (65u + c / 26u) | (65u + c % 26u) << 8;
}
SMH_HD uint32_t grid_row_digits(uint32_t row1, uint32_t *n) {
	if (row1 < 10u) { *n = 1u; return 48u + row1; }
	if (row1 < 100u) { *n = 2u; return (48u + row1 / 10u) | (48u + row1 % 10u) << 8; }
	*n = 3u;
	return (48u + row1 / 100u) | (48u + (row1 / 10u) % 10u) << 8 | (48u + row1 % 10u) << 16;
}
// "<letters><row>" and then "-<digit>" per level into out[16], NUL-padded; digits = digit_1 | digit_2 << 8 | digit_3 << 16.  The text is
// put together in two 64-bit words, low byte first (no array is indexed by a variable: the kernel keeps it in registers).
SMH_HD void grid_text_put(uint64_t *lo, uint64_t *hi, uint32_t *at, uint32_t ch) {
	if (*at < 8u) *lo |= (uint64_t)ch << (8u * *at);
	else *hi |= (uint64_t)ch << (8u * (*at - 8u));
	++*at;
}
SMH_HD void grid_text_words(uint32_t col, uint32_t row1, uint32_t digits, uint32_t levels, uint64_t *plo, uint64_t *phi) {
	uint32_t nl, nr, at = 0u;
	uint64_t lo = 0u, hi = 0u;
	const uint32_t l = grid_letters(col, &nl), r = grid_row_digits(row1, &nr);
	grid_text_put(&lo, &hi, &at, l & 255u);
	if (nl > 1u) grid_text_put(&lo, &hi, &at, (l >> 8) & 255u);
	grid_text_put(&lo, &hi, &at, r & 255u);
	if (nr > 1u) grid_text_put(&lo, &hi, &at, (r >> 8) & 255u);
	if (nr > 2u) grid_text_put(&lo, &hi, &at, (r >> 16) & 255u);
	if (levels >= 1u) { grid_text_put(&lo, &hi, &at, 45u); grid_text_put(&lo, &hi, &at, 48u + (digits & 255u)); }
	if (levels >= 2u) { grid_text_put(&lo, &hi, &at, 45u); grid_text_put(&lo, &hi, &at, 48u + ((digits >> 8) & 255u)); }
	if (levels >= 3u) { grid_text_put(&lo, &hi, &at, 45u); grid_text_put(&lo, &hi, &at, 48u + ((digits >> 16) & 255u)); }
	*plo = lo; *phi = hi;
}
SMH_HD void grid_text(uint32_t col, uint32_t row1, uint32_t digits, uint32_t levels, char out[16]) {
	uint64_t lo, hi;
	grid_text_words(col, row1, digits, levels, &lo, &hi);
	memcpy(out, &lo, 8);
	memcpy(out + 8, &hi, 8);
}
// the keypad digit of level k (1 .. L) from the two idx_L
SMH_HD uint32_t grid_digit(int32_t ix, int32_t iy, uint32_t L, uint32_t k) {
	return (2u - grid_mod3(grid_level(iy, L, k))) * 3u + grid_mod3(grid_level(ix, L, k)) + 1u;
}

// The reference of a point (px, py), already translated, on the axes x and y, as the six little-endian 64-bit words of a
// smhv_grid_ref: x_m, y_m, col | row1 << 32, digit[0 .. 2] and valid in the low four bytes, the text's two halves.
struct GridRefWords { uint64_t w[6]; };
static_assert(sizeof(GridRefWords) == sizeof(smhv_grid_ref), "a reference is six words");
SMH_HD uint64_t grid_bits(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }
SMH_HD GridRefWords grid_ref_words(const GridAxis &x, const GridAxis &y, float px, float py) {
	GridRefWords o;
	const GridIdx ex = grid_index(x, px), ey = grid_index(y, py);
	o.w[0] = grid_bits(grid_finite(ex.g) ? ex.g : 0.0);
	o.w[1] = grid_bits(grid_finite(ey.g) ? ey.g : 0.0);
	o.w[2] = 0u; o.w[3] = 0u; o.w[4] = 0u; o.w[5] = 0u;
	if (!(grid_axis_cell(x, ex, SMHV_GRID_MAX_COLS) && grid_axis_cell(y, ey, SMHV_GRID_MAX_ROWS))) return o;
	const uint32_t L = x.L;
	const uint32_t col = (uint32_t)grid_level(ex.idx, L, 0u), row1 = (uint32_t)grid_level(ey.idx, L, 0u) + 1u;
	const uint32_t d1 = L >= 1u ? grid_digit(ex.idx, ey.idx, L, 1u) : 0u, d2 = L >= 2u ? grid_digit(ex.idx, ey.idx, L, 2u) : 0u,
	               d3 = L >= 3u ? grid_digit(ex.idx, ey.idx, L, 3u) : 0u;
	const uint32_t digits = d1 | d2 << 8 | d3 << 16;
	o.w[2] = (uint64_t)col | (uint64_t)row1 << 32;
	o.w[3] = (uint64_t)(digits | 1u << 24);
	grid_text_words(col, row1, digits, L, &o.w[4], &o.w[5]);
	return o;
}
SMH_HD smhv_grid_ref grid_ref_of(const GridAxis &x, const GridAxis &y, float px, float py) {
	const GridRefWords w = grid_ref_words(x, y, px, py);
	smhv_grid_ref o;
	memcpy(&o, &w, sizeof o);
	return o;
}

}  // namespace smh

#if defined(__HIPCC__)
#include "smh_kernels.h"
namespace smh {
// smhv_batch_grid / smhv_grid_map (k_grid, k_grid_finish) and smhv_batch_grid_refs / smhv_grid_refs (k_grid_refs): launch arguments,
// taken by value at the launch.  The fields window_pass_batch / window_pass_per_call set have the other window passes' names.
struct GridRun {
	FiringRun fr;                        // the heightmap's size and bounds and the viewport (`hm`: non-null = the heightmap branch; `out` is not used)
	const FrameAux *aux;                 // batch, per frame: open
	const smhv_frame_result *res;        // batch, per frame: the minimap rectangle, m/px, the lines
	smhv_grid_result *out;               // the grid slab, at the first frame of the call; cleared ahead of the launch
	uint8_t *img;                        // PAINT: the render slab, at the first frame of the call
	uint8_t *bytes;                      // the planes (null: not asked for): out_w * out_h elements per frame
	uint32_t *cells;
	smhv_grid_refs_result *refs;         // k_grid_refs, batch: the references slab, at the first frame of the call
	const smhv_line *lines;              // k_grid_refs, per call: the explicit lines ...
	smhv_grid_ref *refs_out;             //   ... and two references per line
	uint64_t img_stride, plane_stride;   // out_w * out_h * 4 bytes, out_w * out_h elements
	double mpx;                          // per call: the frame's metres per pixel (valid iff has_mpx)
	double cell_m, origin_m[2], min_px, label_min_px;
	uint32_t mm[4];                      // per call: the minimap rectangle (valid iff has_mm)
	uint32_t out_w, out_h;
	uint32_t levels;
	uint32_t n_lines;                    // per call: of `lines`
	uint32_t per_call, has_mm, has_mpx;  // 1: mpx / has_mpx, mm / has_mm are the call's and aux, res are not read
	uint32_t pal[5];                     // line[0 .. 3], label: R, G, B, a as a little-endian word
};
// the map grid (smh_grid.hip): k_grid<paint, planes> over n frames (at most 65,535), then k_grid_finish over their summaries
hipError_t launch_grid(const GridRun &r, uint32_t n, bool paint, hipStream_t s);
// ... the references: batch (r.refs: n frames, one wave each) or per call (r.lines, r.refs_out: r.n_lines lines, one lane per end)
hipError_t launch_grid_refs(const GridRun &r, uint32_t n, hipStream_t s);
}  // namespace smh
#endif
