// smh_glyph_rule.h -- the rule of "scale labels: text" (include/smh_vision_hip.h): how a label's cell is cut into glyphs, the
// distance of a glyph to a template, the choice among the templates, the text's meters and the frame's anchors.  One text for the
// kernel (smh_labeltext.hip takes the pieces: its lanes share the work of a label), the host helpers (smh_labeltext.inc,
// smh_scalelabels.inc) and a stand-alone host check (tests/glyph_rule_check.cpp compiles this header with g++ and reads whole
// frames through frame_read), hence SMH_HD.  Integers only, except the f64 mean of label_anchors.
#pragma once
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

#define SMH_GLYPH_NONE 0xFFFFu           // best / second of an unmatched glyph, second when no other code exists
#define SMH_GLYPH_NO_TMPL 0xFFu

// An atlas as the device holds it (and the host check): meta = code | w << 8 | h << 16, fg = the template's foreground count,
// rows[t][y] = the template's rows (0 for y >= h).
struct GlyphAtlas {
	uint32_t n, accept_num, accept_den, reserved;
	uint32_t meta[SMHV_ATLAS_MAX_TEMPLATES];
	uint32_t fg[SMHV_ATLAS_MAX_TEMPLATES];
	uint32_t rows[SMHV_ATLAS_MAX_TEMPLATES][32];
};
static_assert(sizeof(GlyphAtlas) == 16u + 128u + 128u + 4096u, "atlas layout");

SMH_HD uint32_t glyph_popc(uint64_t v) { return (uint32_t)__builtin_popcountll(v); }

// ---- glyphs: the runs of non-empty columns.  A row of a cell is 128 bits, (lo, hi): bit x of lo is column x, bit x of hi column 64 + x.
// the first set bit at or after `from` (128: none)
SMH_HD uint32_t glyph_next_bit(uint64_t lo, uint64_t hi, uint32_t from) {
	if (from < 64u) {
		const uint64_t m = lo >> from;
		if (m) return from + (uint32_t)__builtin_ctzll(m);
		from = 64u;
	}
	if (from < 128u) {
		const uint64_t m = hi >> (from - 64u);
		if (m) return from + (uint32_t)__builtin_ctzll(m);
	}
	return 128u;
}

// the first run of set bits at or after `from` -> [*l, *r], both inclusive; false: none
SMH_HD bool glyph_next_run(uint64_t lo, uint64_t hi, uint32_t from, uint32_t *l, uint32_t *r) {
	const uint32_t a = glyph_next_bit(lo, hi, from);
	if (a >= 128u) return false;
	*l = a;
	*r = glyph_next_bit(~lo, ~hi, a) - 1u;
	return true;
}

// bits [l, l + min(w, 32)) of a row, as bits 0 .. of a word
SMH_HD uint32_t glyph_row_bits(uint64_t lo, uint64_t hi, uint32_t l, uint32_t w) {
	const uint64_t v = l < 64u ? ((lo >> l) | (l ? hi << (64u - l) : 0ull)) : (hi >> (l - 64u));
	return (uint32_t)v & (w >= 32u ? 0xFFFFFFFFu : ((1u << w) - 1u));
}

// ---- distance: G (rows g[0, gh)) moved by (dx, dy) against T (rows t[0, th)); plane column x is bit x + 1 of a 64-bit row, the
// plane's rows run from -1 to max(gh, th): 32 + 2 at most either way
SMH_HD uint32_t glyph_shift_distance(const uint32_t *g, uint32_t gh, const uint32_t *t, uint32_t th, int dx, int dy) {
	uint32_t d = 0;
	const int rows = (int)(gh > th ? gh : th) + 1;
	for (int y = -1; y < rows; ++y) {
		const int gy = y - dy;
		const uint64_t a = (gy >= 0 && gy < (int)gh) ? (uint64_t)g[gy] << (1 + dx) : 0ull;
		const uint64_t b = (y >= 0 && y < (int)th) ? (uint64_t)t[y] << 1 : 0ull;
		d += glyph_popc(a ^ b);
	}
	return d;
}

// the (dx, dy) of shift s = 0 .. 8: dy-major, dx-minor
SMH_HD int glyph_shift_dx(uint32_t s) { return (int)(s % 3u) - 1; }
SMH_HD int glyph_shift_dy(uint32_t s) { return (int)(s / 3u) - 1; }

// ---- choice.  A candidate is the key distance << 8 | template index: the least key is the least distance, ties to the lowest index.
SMH_HD uint32_t glyph_key(uint32_t dist, uint32_t t) { return (dist << 8) | t; }
SMH_HD uint32_t glyph_meta_code(uint32_t meta) { return meta & 255u; }
SMH_HD uint32_t glyph_meta_h(uint32_t meta) { return (meta >> 16) & 255u; }
SMH_HD bool glyph_accept(uint32_t best, uint32_t fg, uint32_t num, uint32_t den) { return best * den <= num * fg; }

// one glyph against the whole atlas, one after the other (the kernel spreads the (template, shift) pairs over a wave's lanes)
SMH_HD void glyph_choose(const GlyphAtlas *A, const uint32_t *g, uint32_t gw, uint32_t gh, char *ch, uint16_t *best, uint16_t *second, uint8_t *tmpl) {
	*ch = '?'; *best = SMH_GLYPH_NONE; *second = SMH_GLYPH_NONE; *tmpl = SMH_GLYPH_NO_TMPL;
	if (gw > 32u) return;
	uint32_t win = 0xFFFFFFFFu;
	for (uint32_t t = 0; t < A->n; ++t)
		for (uint32_t s = 0; s < 9u; ++s) {
			const uint32_t k = glyph_key(glyph_shift_distance(g, gh, A->rows[t], glyph_meta_h(A->meta[t]), glyph_shift_dx(s), glyph_shift_dy(s)), t);
			win = k < win ? k : win;
		}
	const uint32_t wt = win & 255u, wcode = glyph_meta_code(A->meta[wt]);
	uint32_t sec = 0xFFFFFFFFu;
	for (uint32_t t = 0; t < A->n; ++t) {
		if (glyph_meta_code(A->meta[t]) == wcode) continue;
		for (uint32_t s = 0; s < 9u; ++s) {
			const uint32_t k = glyph_key(glyph_shift_distance(g, gh, A->rows[t], glyph_meta_h(A->meta[t]), glyph_shift_dx(s), glyph_shift_dy(s)), t);
			sec = k < sec ? k : sec;
		}
	}
	*best = (uint16_t)(win >> 8); *tmpl = (uint8_t)wt;
	*second = sec == 0xFFFFFFFFu ? (uint16_t)SMH_GLYPH_NONE : (uint16_t)(sec >> 8);
	if (glyph_accept(win >> 8, A->fg[wt], A->accept_num, A->accept_den)) *ch = (char)wcode;
}

// ---- text to meters: src/vision/mod.rs:161-173 (rfind('m'), then u32::from_str on what precedes it)
SMH_HD uint32_t label_meters(const char *text, uint32_t len) {
	int p = -1;
	for (uint32_t i = 0; i < len; ++i)
		if (text[i] == 'm') p = (int)i;
	if (p < 0) return 0u;
	int i = (p > 0 && text[0] == '+') ? 1 : 0;
	if (i >= p) return 0u;
	uint64_t v = 0;
	for (; i < p; ++i) {
		const char c = text[i];
		if (c < '0' || c > '9') return 0u;
		v = v * 10u + (uint64_t)(c - '0');
		if (v > 0xFFFFFFFFull) return 0u;
	}
	return (uint32_t)v;
}

// ---- frame: the label filter of src/vision/mod.rs:161-186 and the ladder of mpx_ratio.rs:91-125 on the labels' own widths.
// meters[i] == 0: not a label (`Ok(0) | Err(_) => continue`).  false: label *bad was taken and has no bar (bar_right <= bar_left).
SMH_HD bool label_anchors(const smhv_scale_label *labels, uint32_t n, const uint32_t *meters, smhv_anchors *an, double *mpx, uint32_t *bad) {
	an->n = 0u; an->scales_start_y = 0u;                      // (filled in place: the kernel's *an lies in LDS, and a local indexed by an->n would not stay in registers)
	for (uint32_t k = 0; k < (uint32_t)SMHV_MAX_SCALES; ++k) an->scales[k][0] = an->scales[k][1] = an->scales[k][2] = 0u;
	*mpx = 0.0;
	uint32_t start_y = 0xFFFFFFFFu, cnt = 0u;
	double sum = 0.0;
	for (uint32_t i = 0; i < n && cnt < (uint32_t)SMHV_MAX_SCALES; ++i) {
		if (meters[i] == 0u) continue;
		start_y = labels[i].bottom < start_y ? labels[i].bottom : start_y;
		bool seen = false;
		for (uint32_t k = 0; k < cnt; ++k) seen = seen || an->scales[k][0] == meters[i];
		if (seen) continue;
		if (labels[i].bar_right <= labels[i].bar_left) { *bad = i; return false; }
		const uint32_t width = labels[i].bar_right - labels[i].bar_left;
		an->scales[cnt][0] = meters[i];
		an->scales[cnt][1] = (labels[i].left + labels[i].right) / 2u;
		an->scales[cnt][2] = labels[i].bottom;
		const double ratio = (double)meters[i] / (double)width;
		sum = cnt ? sum + ratio : ratio;
		++cnt;
	}
	an->n = cnt;
	an->scales_start_y = cnt ? start_y : 0u;
	*mpx = cnt == 0u ? 0.0 : (cnt == 1u ? sum : sum / (double)cnt);
	return true;
}

// ---- a whole label and a whole frame, one step after the other: the host's way through the rule
// the rows of a cell (SMHV_LABEL_CROP_W bytes each) as bits, columns [0, w) and rows [0, h) only -> the columns' occupancy
SMH_HD void label_row_masks(const uint8_t *cell, uint32_t w, uint32_t h, uint64_t lo[32], uint64_t hi[32], uint64_t *occ_lo, uint64_t *occ_hi) {
	*occ_lo = *occ_hi = 0ull;
	for (uint32_t y = 0; y < 32u; ++y) {
		lo[y] = hi[y] = 0ull;
		if (y >= h) continue;
		for (uint32_t x = 0; x < w && x < 128u; ++x)
			if (cell[y * SMHV_LABEL_CROP_W + x] != 255u) (x < 64u ? lo[y] : hi[y]) |= 1ull << (x & 63u);
		*occ_lo |= lo[y]; *occ_hi |= hi[y];
	}
}

// the glyph of columns [l, r] -> its rows g[0, *gh) (g[y] = 0 beyond), its width; a glyph wider than 32 columns has no rows
SMH_HD void label_glyph(const uint64_t lo[32], const uint64_t hi[32], uint32_t l, uint32_t r, uint32_t g[32], uint32_t *gw, uint32_t *gh) {
	*gw = r - l + 1u; *gh = 0u;
	for (uint32_t y = 0; y < 32u; ++y) g[y] = 0u;
	if (*gw > 32u) return;
	uint32_t top = 32u, bot = 0u;
	for (uint32_t y = 0; y < 32u; ++y)
		if (glyph_row_bits(lo[y], hi[y], l, *gw)) { top = y < top ? y : top; bot = y; }
	*gh = bot - top + 1u;                                      // (a run of non-empty columns has a non-empty row)
	for (uint32_t y = top; y <= bot; ++y) g[y - top] = glyph_row_bits(lo[y], hi[y], l, *gw);
}

SMH_HD void label_read(const GlyphAtlas *A, const uint8_t *cell, const smhv_scale_label *lb, smhv_label_text_entry *out) {
	memset(out, 0, sizeof *out);
	uint64_t lo[32], hi[32], olo, ohi;
	label_row_masks(cell, lb->right - lb->left, lb->bottom - lb->top, lo, hi, &olo, &ohi);
	uint32_t n = 0, l = 0, r = 0;
	for (uint32_t from = 0; glyph_next_run(olo, ohi, from, &l, &r); from = r + 1u) {
		if (n < (uint32_t)SMHV_LABEL_MAX_GLYPHS) {
			uint32_t g[32], gw, gh;
			label_glyph(lo, hi, l, r, g, &gw, &gh);
			glyph_choose(A, g, gw, gh, &out->text[n], &out->best[n], &out->second[n], &out->tmpl[n]);
		}
		++n;
	}
	out->n_glyphs = n;
	if (n > (uint32_t)SMHV_LABEL_MAX_GLYPHS) {
		memset(out, 0, sizeof *out);
		out->n_glyphs = n; out->flags = SMHV_LABEL_TEXT_TOO_MANY;
		return;
	}
	out->meters = label_meters(out->text, n);
}

// cells: the frame's SMHV_LABEL_FRAME_CROP_BYTES
SMH_HD void frame_read(const GlyphAtlas *A, const smhv_scale_label_frame *f, const uint8_t *cells, smhv_label_text_frame *out) {
	memset(out, 0, sizeof *out);
	const uint32_t n = f->n < (uint32_t)SMHV_MAX_SCALE_LABELS ? f->n : (uint32_t)SMHV_MAX_SCALE_LABELS;
	uint32_t meters[SMHV_MAX_SCALE_LABELS], bad = 0;
	for (uint32_t i = 0; i < n; ++i) {
		label_read(A, cells + (size_t)i * SMHV_LABEL_CROP_BYTES, &f->label[i], &out->label[i]);
		meters[i] = out->label[i].meters;
	}
	out->n = n;
	if (!label_anchors(f->label, n, meters, &out->anchors, &out->mpx, &bad)) { memset(&out->anchors, 0, sizeof out->anchors); out->mpx = 0.0; }
	out->has = out->anchors.n ? 1u : 0u;
}

// ---- templates: the conditions of the header.  0: fine; otherwise what is wrong, as a string
SMH_HD const char *glyph_template_fault(const smhv_glyph_template *t) {
	if (t->code < 0x21u || t->code > 0x7Eu || t->code == (uint8_t)'?') return "code is not printable ASCII 0x21 .. 0x7E, or is '?'";
	if (t->w < 1u || t->w > 32u || t->h < 1u || t->h > 32u) return "w and h must lie in 1 .. 32";
	if (t->reserved) return "reserved is not 0";
	const uint32_t mask = t->w >= 32u ? 0xFFFFFFFFu : ((1u << t->w) - 1u);
	uint32_t any = 0;
	for (uint32_t y = 0; y < 32u; ++y) {
		if (y >= t->h && t->rows[y]) return "bits below the box";
		if (t->rows[y] & ~mask) return "bits right of the box";
		any |= t->rows[y];
	}
	if (!t->rows[0] || !t->rows[t->h - 1u] || !(any & 1u) || !((any >> (t->w - 1u)) & 1u)) return "the box is not tight";
	return nullptr;
}

SMH_HD void glyph_atlas_fill(GlyphAtlas *A, const smhv_glyph_template *t, uint32_t n, uint32_t num, uint32_t den) {
	memset(A, 0, sizeof *A);
	A->n = n; A->accept_num = num; A->accept_den = den;
	for (uint32_t i = 0; i < n; ++i) {
		A->meta[i] = (uint32_t)t[i].code | ((uint32_t)t[i].w << 8) | ((uint32_t)t[i].h << 16);
		for (uint32_t y = 0; y < 32u; ++y) { A->rows[i][y] = t[i].rows[y]; A->fg[i] += glyph_popc(t[i].rows[y]); }
	}
}

}  // namespace smh
