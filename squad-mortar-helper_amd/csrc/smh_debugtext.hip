// smh_debugtext.hip -- the vision debugger and the Debug menu's text of the map view (gfx950, wave64).
//   k_probe        src/ui/debug.rs:357-385: the pixel under a window position and everything the debugger prints about it -> the probe
//                  slab (SMHV_MAX_PROBES smhv_probe per frame)
//   k_debug_plan   a frame's item list in paint order: the call's text runs, the caption, and per valid probe the window's fill, its
//                  text (built here), the swatch and the pixel frame -- each with the window bounding box the draw culls by
//   k_debug_draw   the pixel rules over a finished image of the map view (the render slab)
//
// The semantics are spelt out in include/smh_vision_hip.h ("map view: debug text and the vision debugger"); every operation below
// that feeds a probe or a pixel is one of its operations, in its order, unfused (-ffp-contract=off, IEEE division).
//
// k_probe: one lane per (frame, probe): one dword gathered from the pitched ui slab, the arithmetic, two 16-byte stores.
// k_debug_plan: one workgroup per frame, one lane per item source.  A probe's string is built in LDS, a number from its last digit
// backwards, and leaves for the frame's pool in dwords.  An item has a FIXED place in the list (run i, the caption, probe k's four
// parts): what is absent is an item of kind NONE with an empty box, so the list's order is the paint order without a compaction.
// k_debug_draw: output-driven, k_label_draw's shape.  A workgroup of four waves takes a tile of 64 x 32 pixels of one frame, a
// wave a row at a time, a lane a column.  It tests the frame's items against the tile (one lane an item), compacts the survivors
// in order into LDS and leaves when there are none -- almost every tile -- without touching the image.  A lane walks the list from
// its end and takes the first hit: what was painted last.  Only painted pixels are stored.  The font (679 bytes) sits in LDS.
#include "smh_device.h"
#include "smh_font5x7_ascii.h"

namespace smh {

#define SMH_DBG_TW 64u
#define SMH_DBG_TH 32u
#define SMH_DBG_WAVES 4u
static_assert(sizeof(smhv_probe) == 32 && sizeof(smhv_text_run) == 84 && sizeof(smhv_probe_point) == 8, "the layouts are public");
static_assert(sizeof(DebugItem) == 72, "k_debug_draw copies an item as 18 dwords");
static_assert(SMH_DBG_ITEMS <= 64u * SMH_DBG_WAVES, "k_debug_draw: a lane per item");
static_assert(SMHV_TEXT_MAX_RUNS + 1u + SMHV_MAX_PROBES <= 128u, "k_debug_plan: a lane per run, one for the caption, one per probe");

__constant__ uint8_t c_text_font[SMH_TEXT_FONT_GLYPHS][SMH_TEXT_FONT_ROWS] = SMH_FONT5X7_ASCII_TABLE;
__device__ const uint8_t c_caption[] = "No minimap bounds detected or we don't need to detect them";
#define SMH_DBG_CAPTION_LEN 58u
static_assert(sizeof(c_caption) == SMH_DBG_CAPTION_LEN + 1u, "the caption's length");

__device__ __forceinline__ bool dbg_finite(float v) { return v - v == 0.0f; }

// ---- the probe ----
__global__ void __launch_bounds__(64) k_probe(Geom g, DebugRun r, uint32_t n_frames) {
	const uint32_t id = blockIdx.x * 64u + threadIdx.x;
	const uint32_t f = id / SMHV_MAX_PROBES, k = id % SMHV_MAX_PROBES;
	if (f >= n_frames) return;
	uint32_t w0 = 0u, w1 = 0u, w2 = 0u, w3 = 0u, w4 = 0u, w5 = 0u, w6 = 0u;
	if (k < r.n_points && r.aux[f].open) {
		const smhv_probe_point pt = r.points[k];
		const bool away = pt.x == 3.402823466e+38f && pt.y == 3.402823466e+38f;
		const float ix = (pt.x - r.tx) / r.sw, iy = (pt.y - r.ty) / r.sh;
		const uint32_t px = f2u(ix), py = f2u(iy);
		if (!away && !(ix < 0.0f || iy < 0.0f) && px < g.rw && py < g.rh) {
			const uint32_t p = ((const uint32_t *)(r.ui + (size_t)f * g.ui_stride + (size_t)py * g.ui_pitch))[g.m_xoff + px];
			const uint32_t r8 = p & 255u, g8 = (p >> 8) & 255u, b8 = (p >> 16) & 255u;
			// util/src/image.rs:159-187, the operations of marker_exact (smh_device.h)
			const float rf = (float)r8 / 255.0f, gf = (float)g8 / 255.0f, bf = (float)b8 / 255.0f;
			const float mx = fmaxf(rf, fmaxf(gf, bf));
			const float mn = fminf(rf, fminf(gf, bf));
			const float delta = mx - mn;
			float h;
			if (mx == mn) h = 0.0f;
			else if (mx == rf) h = 60.0f * ((gf - bf) / delta);
			else if (mx == gf) h = 60.0f * (((bf - rf) / delta) + 2.0f);
			else h = 60.0f * (((rf - gf) / delta) + 4.0f);
			if (h < 0.0f) h = h + 360.0f;
			const float sf = (100.0f * delta) / mx;                  // NaN when mx == 0 -> 0
			const float vf = 100.0f * mx;
			uint32_t hu = f2u(h); hu = hu > 65535u ? 65535u : hu;
			uint32_t su = f2u(sf); su = su > 255u ? 255u : su;
			uint32_t vu = f2u(vf); vu = vu > 255u ? 255u : vu;
			const uint32_t mono = 2u * (absdiff(r8, g8) + absdiff(r8, b8) + absdiff(g8, b8));
			const uint32_t bright = min(r8, min(g8, b8));
			uint32_t bits = 0u;
#define SMH_TEAM(T, MH, MS, MV)                                                                                                  \
	bits |= (uint32_t)(absdiff(MH, hu) <= SMH_HSV_HUE_TOLERANCE) << (3u * (T));                                                   \
	bits |= (uint32_t)(su >= SMH_HSV_MIN_SAT && (absdiff(MS, su) <= SMH_HSV_SAT_TOLERANCE ||                                      \
	                                            (uint32_t)abs((int)su - ((int)(MS) - SMH_PLAYER_DIR_ARC_SAT)) <= SMH_HSV_SAT_TOLERANCE)) \
	        << (3u * (T) + 1u);                                                                                                   \
	bits |= (uint32_t)(absdiff(MV, vu) <= SMH_HSV_VIB_TOLERANCE) << (3u * (T) + 2u)
			SMH_TEAM(0u, SMH_ALPHA_H, SMH_ALPHA_S, SMH_ALPHA_V);
			SMH_TEAM(1u, SMH_BRAVO_H, SMH_BRAVO_S, SMH_BRAVO_V);
			SMH_TEAM(2u, SMH_CHARLIE_H, SMH_CHARLIE_S, SMH_CHARLIE_V);
#undef SMH_TEAM
			w0 = 1u; w1 = px; w2 = py;
			w3 = r8 | (g8 << 8) | (b8 << 16) | (luma8(r8, g8, b8) << 24);
			w4 = hu | (su << 16) | (vu << 24);
			w5 = mono | (bright << 16);
			w6 = bits;
		}
	}
	uint4 *out = (uint4 *)&r.probes[(size_t)f * SMHV_MAX_PROBES + k];
	out[0] = make_uint4(w0, w1, w2, w3);
	out[1] = make_uint4(w4, w5, w6, 0u);
}

// ---- the plan ----
// the box of [lo, hi) in window pixels, grown by the rounding of coordinates of this size, clamped to the window; a NaN gives an
// empty box (fmaxf(NaN, 0) is 0 at both ends)
__device__ __forceinline__ void dbg_box(DebugItem &it, float lox, float loy, float hix, float hiy, float W, float H) {
	const float mx = 2.0f + 1e-6f * fmaxf(fabsf(lox), fabsf(hix)), my = 2.0f + 1e-6f * fmaxf(fabsf(loy), fabsf(hiy));
	it.x0 = (int32_t)fminf(fmaxf(floorf(lox - mx), 0.0f), W);
	it.x1 = (int32_t)fminf(fmaxf(ceilf(hix + mx), 0.0f), W);
	it.y0 = (int32_t)fminf(fmaxf(floorf(loy - my), 0.0f), H);
	it.y1 = (int32_t)fminf(fmaxf(ceilf(hiy + my), 0.0f), H);
}
__device__ __forceinline__ DebugItem dbg_none() {
	DebugItem it;
	it.text = nullptr;
	it.ax = it.ay = it.bx = it.by = 0.0f;
	it.x0 = it.y0 = it.x1 = it.y1 = 0;
	it.color = 0u; it.kind = SMH_DBG_NONE; it.n_lines = 0u; it.pad = 0u;
	for (uint32_t i = 0; i < 8u; ++i) { it.off[i] = 0; it.len[i] = 0; }
	return it;
}
// a text item at anchor (px, py): its line table is filled in already
__device__ __forceinline__ void dbg_text_item(DebugItem &it, const uint8_t *text, float px, float py, uint32_t color, uint32_t S, float W, float H) {
	if (!(dbg_finite(px) && dbg_finite(py))) return;               // (stays NONE: a run whose anchor is not finite paints nothing)
	uint32_t widest = 0u;
	for (uint32_t i = 0; i < it.n_lines; ++i) widest = max(widest, (uint32_t)it.len[i]);
	it.text = text; it.ax = px; it.ay = py; it.color = color; it.kind = SMH_DBG_TEXT_ITEM;
	dbg_box(it, px, py, px + (float)(6u * S * widest), py + (float)(9u * S * it.n_lines), W, H);
}
__device__ __forceinline__ void dbg_rect_item(DebugItem &it, uint32_t kind, float ax, float ay, float bx, float by, uint32_t color, float W, float H) {
	it.ax = ax; it.ay = ay; it.bx = bx; it.by = by; it.color = color; it.kind = kind;
	dbg_box(it, ax, ay, bx, by, W, H);
}
__device__ __forceinline__ void dbg_str(uint8_t *s, uint32_t &n, const char *lit) {
	for (; *lit; ++lit) s[n++] = (uint8_t)*lit;
}
// an unsigned decimal up to 65535, from the last digit backwards
__device__ __forceinline__ void dbg_num(uint8_t *s, uint32_t &n, uint32_t v) {
	const uint32_t nd = 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u);
	for (uint32_t i = 0; i < nd; ++i) {
		s[n + nd - 1u - i] = (uint8_t)(48u + v % 10u);
		v /= 10u;
	}
	n += nd;
}
__device__ __forceinline__ void dbg_three(uint8_t *s, uint32_t &n, uint32_t a, uint32_t b, uint32_t c) {
	s[n++] = '[';
	dbg_num(s, n, a); s[n++] = ','; s[n++] = ' ';
	dbg_num(s, n, b); s[n++] = ','; s[n++] = ' ';
	dbg_num(s, n, c);
	s[n++] = ']';
}
__device__ __forceinline__ void dbg_bools(uint8_t *s, uint32_t &n, uint32_t bits) {
	s[n++] = '[';
	for (uint32_t k = 0; k < 3u; ++k) {
		dbg_str(s, n, (bits >> k) & 1u ? "true" : "false");
		if (k < 2u) { s[n++] = ','; s[n++] = ' '; }
	}
	s[n++] = ']';
}

__global__ void __launch_bounds__(128) k_debug_plan(DebugRun r) {
	__shared__ __attribute__((aligned(4))) uint8_t s_txt[SMHV_MAX_PROBES][SMH_DBG_TEXT];
	const uint32_t f = blockIdx.x, tid = threadIdx.x;
	DebugItem *items = r.items + (size_t)f * SMH_DBG_ITEMS;
	uint8_t *pool = r.pool + (size_t)f * (SMHV_MAX_PROBES * SMH_DBG_TEXT);
	const bool open = r.aux[f].open != 0u;
	const float W = (float)r.out_w, H = (float)r.out_h;
	const uint32_t S = r.scale;
	if (tid < r.n_runs) {
		DebugItem it = dbg_none();
		if (open) {
			const smhv_text_run *run = &r.runs[tid];
			const uint32_t n = min(run->n, SMHV_TEXT_MAX_BYTES);
			uint32_t line = 0u, start = 0u;
			for (uint32_t i = 0; i <= n; ++i)
				if (i == n || run->text[i] == '\n') {
					if (line < SMHV_TEXT_MAX_LINES) { it.off[line] = (uint8_t)start; it.len[line] = (uint8_t)(i - start); }
					++line; start = i + 1u;
				}
			it.n_lines = min(line, SMHV_TEXT_MAX_LINES);
			float px = run->x, py = run->y;
			if (run->flags & SMHV_TEXT_MAP_COORDS) { px = px * r.sw + r.tx; py = py * r.sh + r.ty; }
			const uint32_t color = (uint32_t)run->rgba[0] | ((uint32_t)run->rgba[1] << 8) | ((uint32_t)run->rgba[2] << 16) | 0xFF000000u;
			dbg_text_item(it, run->text, px, py, color, S, W, H);
		}
		items[tid] = it;
	} else if (tid == SMHV_TEXT_MAX_RUNS) {
		DebugItem it = dbg_none();
		if (open && (r.flags & SMHV_DEBUG_MINIMAP_CAPTION) && r.res[f].has_minimap == 0u) {
			it.n_lines = 1u; it.len[0] = (uint8_t)SMH_DBG_CAPTION_LEN;
			dbg_text_item(it, c_caption, 10.0f, (H - 10.0f) - (float)(9u * S), 0xFF0000FFu, S, W, H);
		}
		items[r.n_runs] = it;
	} else if (tid > SMHV_TEXT_MAX_RUNS && tid - (SMHV_TEXT_MAX_RUNS + 1u) < r.n_points) {
		const uint32_t k = tid - (SMHV_TEXT_MAX_RUNS + 1u);
		DebugItem fill = dbg_none(), text = dbg_none(), swatch = dbg_none(), frame = dbg_none();
		const uint32_t *pw = (const uint32_t *)&r.probes[(size_t)f * SMHV_MAX_PROBES + k];
		uint8_t *s = s_txt[k];
		uint32_t n = 0u;
		if (open && (r.flags & SMHV_DEBUG_DRAW_PROBES) && pw[0]) {
			const uint32_t w3 = pw[3], w4 = pw[4], w5 = pw[5], bits = pw[6];
			const uint32_t r8 = w3 & 255u, g8 = (w3 >> 8) & 255u, b8 = (w3 >> 16) & 255u;
			uint32_t line = 0u;
#define SMH_DBG_LINE_BEGIN() text.off[line] = (uint8_t)n
#define SMH_DBG_LINE_END() do { text.len[line] = (uint8_t)(n - text.off[line]); ++line; if (line < 8u) s[n++] = '\n'; } while (0)
			SMH_DBG_LINE_BEGIN(); dbg_str(s, n, "RGB "); dbg_three(s, n, r8, g8, b8); SMH_DBG_LINE_END();
			SMH_DBG_LINE_BEGIN(); dbg_str(s, n, "HSV "); dbg_three(s, n, w4 & 0xFFFFu, (w4 >> 16) & 255u, w4 >> 24); SMH_DBG_LINE_END();
			SMH_DBG_LINE_BEGIN(); dbg_str(s, n, "Luma8 "); dbg_num(s, n, w3 >> 24); SMH_DBG_LINE_END();
			SMH_DBG_LINE_BEGIN(); dbg_str(s, n, "OCRPixelSimilarity "); dbg_num(s, n, w5 & 0xFFFFu); SMH_DBG_LINE_END();
			SMH_DBG_LINE_BEGIN(); dbg_str(s, n, "OCRBrightness "); dbg_num(s, n, (w5 >> 16) & 255u); SMH_DBG_LINE_END();
			SMH_DBG_LINE_BEGIN(); dbg_str(s, n, "AlphaMarker "); dbg_bools(s, n, bits); SMH_DBG_LINE_END();
			SMH_DBG_LINE_BEGIN(); dbg_str(s, n, "BravoMarker "); dbg_bools(s, n, bits >> 3); SMH_DBG_LINE_END();
			SMH_DBG_LINE_BEGIN(); dbg_str(s, n, "CharlieMarker "); dbg_bools(s, n, bits >> 6); SMH_DBG_LINE_END();
#undef SMH_DBG_LINE_BEGIN
#undef SMH_DBG_LINE_END
			text.n_lines = 8u;
			uint32_t C = 0u;
			for (uint32_t i = 0; i < 8u; ++i) C = max(C, (uint32_t)text.len[i]);
			const smhv_probe_point pt = r.points[k];
			const float Wd = (float)(6u * S * C + 16u), Hd = (float)(34u + 72u * S);
			float wx = pt.x + 15.0f, wy = pt.y + 15.0f;
			if (wx + Wd > W || wy + Hd > H) { wx = (pt.x - Wd) - 5.0f; wy = (pt.y - Hd) - 5.0f; }
			dbg_rect_item(fill, SMH_DBG_FILL, wx, wy, wx + Wd, wy + Hd, 0xFF0F0F0Fu, W, H);
			dbg_text_item(text, pool + k * SMH_DBG_TEXT, wx + 8.0f, wy + 26.0f, 0xFFFFFFFFu, S, W, H);
			dbg_rect_item(swatch, SMH_DBG_FILL, wx + 8.0f, wy + 8.0f, (wx + Wd) - 8.0f, wy + 18.0f, (w3 & 0x00FFFFFFu) | 0xFF000000u, W, H);
			const float pwf = floorf(r.sw), phf = floorf(r.sh);
			float ax = pt.x, ay = pt.y;
			if (pwf > 1.0f) ax = ax - fmodf(ax, pwf);
			if (phf > 1.0f) ay = ay - fmodf(ay, phf);
			const float c0x = ax - pwf, c0y = ay - phf, c1x = ax + phf, c1y = ay + phf;
			const bool dark = ((float)r8 * 0.299f + (float)g8 * 0.587f) + (float)b8 * 0.114f > 186.0f;
			dbg_rect_item(frame, SMH_DBG_FRAME, fminf(c0x, c1x), fminf(c0y, c1y), fmaxf(c0x, c1x), fmaxf(c0y, c1y), dark ? 0xFF000000u : 0xFFFFFFFFu, W, H);
		}
		for (; n < SMH_DBG_TEXT; ++n) s[n] = 0;
		DebugItem *o = items + r.n_runs + 1u + 4u * k;
		o[0] = fill; o[1] = text; o[2] = swatch; o[3] = frame;
	}
	__syncthreads();
	const uint32_t words = r.n_points * (SMH_DBG_TEXT / 4u);
	for (uint32_t i = tid; i < words; i += 128u) ((uint32_t *)pool)[i] = ((const uint32_t *)&s_txt[0][0])[i];
}

// ---- the draw ----
__global__ void __launch_bounds__(64 * SMH_DBG_WAVES) k_debug_draw(DebugRun r) {
	__shared__ DebugItem s_item[SMH_DBG_ITEMS];
	__shared__ uint8_t s_font[SMH_TEXT_FONT_GLYPHS * SMH_TEXT_FONT_ROWS + 1];
	__shared__ uint32_t s_wave_n[SMH_DBG_WAVES], s_slot[SMH_DBG_ITEMS];

	const uint32_t f = blockIdx.z, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
	if (!r.aux[f].open) return;                                    // (uniform) a closed frame gets nothing
	const uint32_t n_items = r.n_runs + 1u + 4u * r.n_points;       // (uniform, <= SMH_DBG_ITEMS: the host checks the counts)
	const DebugItem *items = r.items + (size_t)f * SMH_DBG_ITEMS;
	const int32_t tile_x = (int32_t)(blockIdx.x * SMH_DBG_TW), tile_y = (int32_t)(blockIdx.y * SMH_DBG_TH);

	bool keep = false;
	if (tid < n_items) {
		const DebugItem *it = &items[tid];
		const int32_t x0 = it->x0, y0 = it->y0, x1 = it->x1, y1 = it->y1;
		keep = it->kind != SMH_DBG_NONE && x0 < x1 && y0 < y1 && x0 < tile_x + (int32_t)SMH_DBG_TW && x1 > tile_x && y0 < tile_y + (int32_t)SMH_DBG_TH && y1 > tile_y;
	}
	const unsigned long long bal = __ballot(keep);
	if (lane == 0u) s_wave_n[wave] = (uint32_t)__popcll(bal);
	__syncthreads();
	uint32_t base = 0, n_list = 0;
	for (uint32_t w = 0; w < SMH_DBG_WAVES; ++w) {
		if (w < wave) base += s_wave_n[w];
		n_list += s_wave_n[w];
	}
	if (n_list == 0u) return;                                      // (uniform) almost every tile: nothing of the image is touched
	if (keep) s_slot[base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = tid;
	for (uint32_t i = tid; i < SMH_TEXT_FONT_GLYPHS * SMH_TEXT_FONT_ROWS; i += 64u * SMH_DBG_WAVES) s_font[i] = ((const uint8_t *)c_text_font)[i];
	__syncthreads();
	for (uint32_t k = tid; k < n_list * 18u; k += 64u * SMH_DBG_WAVES) {
		const uint32_t i = k / 18u, w = k - i * 18u;
		((uint32_t *)&s_item[i])[w] = ((const uint32_t *)&items[s_slot[i]])[w];
	}
	__syncthreads();

	const uint32_t X = (uint32_t)tile_x + lane;
	if (X >= r.out_w) return;
	const float fS = (float)r.scale;
	const float cx = (float)X + 0.5f;
	uint32_t *img = (uint32_t *)(r.img + (size_t)f * r.img_stride);
	for (uint32_t j = 0; j < SMH_DBG_TH / SMH_DBG_WAVES; ++j) {
		const uint32_t Y = (uint32_t)tile_y + j * SMH_DBG_WAVES + wave;
		if (Y >= r.out_h) break;                                   // (wave-uniform)
		const float cy = (float)Y + 0.5f;
		bool done = false;
		uint32_t color = 0u;
		for (uint32_t li = n_list; li-- > 0u && !done;) {
			const DebugItem *it = &s_item[li];
			if ((int32_t)X < it->x0 || (int32_t)X >= it->x1 || (int32_t)Y < it->y0 || (int32_t)Y >= it->y1) continue;
			bool hit = false;
			if (it->kind == SMH_DBG_TEXT_ITEM) {
				const float u = (cx - it->ax) / fS, v = (cy - it->ay) / fS;
				const float fu = floorf(u), fv = floorf(v);
				if (fu >= 0.0f && fv >= 0.0f && fu < 65536.0f && fv < 65536.0f) {
					const uint32_t iu = (uint32_t)fu, iv = (uint32_t)fv;
					const uint32_t line = iv / 9u, ch = iu / 6u;
					if (line < it->n_lines && ch < it->len[line]) {
						const uint32_t col = iu - ch * 6u, row = iv - line * 9u;
						if (col < 5u && row >= 1u && row <= 7u) {
							const int gi = smh_text_font_index(it->text[it->off[line] + ch]);
							const uint32_t bits = s_font[(uint32_t)(gi < 0 ? 0 : gi) * SMH_TEXT_FONT_ROWS + (row - 1u)];   // (the host lets no other byte in; a blank keeps the read in the table)
							hit = ((bits >> (4u - col)) & 1u) != 0u;
						}
					}
				}
			} else {
				const float ax = it->ax, ay = it->ay, bx = it->bx, by = it->by;
				hit = ax <= cx && cx < bx && ay <= cy && cy < by;
				if (it->kind == SMH_DBG_FRAME) hit = hit && !(ax + 1.0f <= cx && cx < bx - 1.0f && ay + 1.0f <= cy && cy < by - 1.0f);
			}
			if (hit) { done = true; color = it->color; }
		}
		if (done) img[(size_t)Y * r.out_w + X] = color;
	}
}

// at most 65,535 frames per launch of the draw (the grid's third dimension); the probe and the plan go with it chunk by chunk
hipError_t launch_debug_text(const Geom &g, const DebugRun &run, uint32_t n, hipStream_t s) {
	const uint32_t tiles_x = (run.out_w + SMH_DBG_TW - 1u) / SMH_DBG_TW, tiles_y = (run.out_h + SMH_DBG_TH - 1u) / SMH_DBG_TH;
	// nothing can be painted without a run, the caption or the probes' picture: the probe slab alone is written then
	const bool draw = run.img && (run.n_runs || (run.flags & SMHV_DEBUG_MINIMAP_CAPTION) || ((run.flags & SMHV_DEBUG_DRAW_PROBES) && run.n_points));
	for (uint32_t done = 0; done < n;) {
		const uint32_t k = n - done < 65535u ? n - done : 65535u;
		DebugRun r = run;
		r.ui += (size_t)done * g.ui_stride;
		r.aux += done;
		r.res += done;
		r.probes += (size_t)done * SMHV_MAX_PROBES;
		hipLaunchKernelGGL(k_probe, dim3((k * SMHV_MAX_PROBES + 63u) / 64u), dim3(64), 0, s, g, r, k);
		if (draw) {
			r.items += (size_t)done * SMH_DBG_ITEMS;
			r.pool += (size_t)done * (SMHV_MAX_PROBES * SMH_DBG_TEXT);
			r.img += (size_t)done * r.img_stride;
			hipLaunchKernelGGL(k_debug_plan, dim3(k), dim3(128), 0, s, r);
			hipLaunchKernelGGL(k_debug_draw, dim3(tiles_x, tiles_y, k), dim3(64u * SMH_DBG_WAVES), 0, s, r);
		}
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return e;
		done += k;
	}
	return hipSuccess;
}

}  // namespace smh
