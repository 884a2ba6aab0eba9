// smh_render.hip -- the app's map view at any viewport (gfx950, wave64).
//   k_render_map<form, waves>    src/ui/map.rs:209-273 (map::render): the ui_map as a nearest-filtered quad, the heightmap overlay
//                                through the viewport (src/ui/heightmaps.rs:794-826), the marker lines (src/ui/markers.rs:28-30)
//
// The f32 restatement of the draw is spelt out in include/smh_vision_hip.h ("map view"); every operation below that feeds a
// pixel is one of its operations, in its order, unfused (-ffp-contract=off, IEEE division).  Where a value comes from (global
// memory, LDS, a register computed once per column) is this file's business; how it is combined is the header's.
//
// Output-driven.  A workgroup owns a tile of SMH_RND_TW x SMH_RND_TH output pixels of one frame at a time; a wave owns a
// row of it at a time, a lane the four pixels lane, lane + 64, lane + 128, lane + 192 of that row: everything that depends on the
// column alone (the quad's texel column, the overlay's tap columns and weights: two IEEE divisions per pixel) is computed once
// and reused for the tile's rows, and every load, gather and store instruction of a wave covers 64 CONSECUTIVE pixels
// (a store is 256 contiguous bytes).  A lane per four consecutive pixels -- 16-byte stores -- was tried first and was slower: each
// gather instruction then spans four times the cache lines, and every line is visited by four instructions instead of one (an
// earlier form of this file; its figures are not reproducible from the tree and are not quoted).
//   per-frame state   open, minimap rectangle, line count: loaded through uniform addresses (scalar registers)
//   lines             the frame's lines are brought through the viewport and culled against the tile once per workgroup into an
//                     LDS list (most tiles see none); the pixel loop walks that list from its end: the last line that paints wins
//   map               nearest sampling gathers exactly the texels it shows (a minified map skips rows and columns)
//   overlay taps      three forms, chosen by the host per call (launch_render_map):
//                     <GATHER> gathers: a lane's 16 texels, then their 16 colours, all in flight together
//                     <STAGE>  the band's texel footprint -- a contiguous rectangle of the heightmap -- is read with coalesced row
//                              loads, looked up ONCE per texel in the colour table and kept in LDS as colours; the taps read
//                              them there.  A band whose footprint exceeds the launch's LDS takes the gathers (decided per band,
//                              uniformly: there is no footprint the kernel cannot draw)
//                     <TABLE>  persistent workgroups of 16 waves, one per CU, keep the heightmap's colour table in LDS in 16 bits
//                              per colour (128 KB: k_hm_lut16) and take tiles in turn: the texels are gathered, their four
//                              colours per pixel come out of LDS instead of a different 128-byte line of L2 per lane
//                     The gathers look the colour up per tap in the heightmap's 65,536-entry table (k_hm_lut): four lookups per
//                     pixel, against texels-per-pixel lookups of the staged form.  The host would take the staged form up to
//                     SMH_RND_STAGE_RATIO texels per pixel and the table form above; the plain gathers are kept for comparison.
//   k_render_map_layers<form, waves>   the same picture with the layers of smhv_batch_render_layers / smhv_render_map_layers (the
//                     header's "map view: layers"): caller's primitives below and above the marker lines, the minimap bounds, and a
//                     debug view as the quad's texture.  One body (render_map_body<.., LAYERS>) serves both kernels; with LAYERS
//                     false every line of the layers is compiled out, so k_render_map is the kernel it was.  Lines, primitives and
//                     the bounds go through the viewport once per workgroup into ONE ordered LDS list (below-prims, marker lines,
//                     foreground prims, bounds); the pixel loop walks it from its end and takes the first hit, which is the paint
//                     order.  An item is 32 bytes, the list at most 256 + 256 + 1 items = 16.4 KB: beside the table form's 128 KB
//                     that is 144.5 KB of the CU's 160 KB, one workgroup per CU as before; the four-wave forms (at most 48 KB of
//                     staging) still fit two.
#include "smh_device.h"
#include "smh_firing.h"

namespace smh {

#define SMH_RND_TW 256u          // tile width: 64 lanes x 4 pixels
#define SMH_RND_TH 32u           // tile height; a workgroup of WAVES waves draws WAVES rows (a band) at a time
#define SMH_RND_BAND 4u          // rows of a band of the four-wave forms (what the staged form's LDS is sized for)
#define SMH_RND_MAX_BANDS 8u
#define SMH_RND_FORM_GATHER 0
#define SMH_RND_FORM_STAGE 1
#define SMH_RND_FORM_TABLE 2
#define SMH_RND_TABLE_WAVES 16u
static_assert(SMH_RND_MAX_LINES == SMHV_RENDER_MAX_LINES, "the LDS line list holds what the runtime admits");

struct RndLine { float px, py, dx, dy, len2; uint32_t color; };
// an entry of the layers' list: a line as RndLine (a, b = P0; c, d = P1 - P0), or a rectangle (a, b = the lesser corner; c, d = the
// greater one; kind = SMHV_PRIM_RECT)
struct RndItem { float a, b, c, d, len2; uint32_t color, kind, pad; };
static_assert(sizeof(RndItem) == 32, "two 16-byte LDS reads per item");
static_assert(sizeof(smhv_render_prim) == 24, "the prim's layout is public");
template <bool LAYERS> struct RndListOf { typedef RndLine T; static constexpr uint32_t N = SMH_RND_MAX_LINES; };
template <> struct RndListOf<true> { typedef RndItem T; static constexpr uint32_t N = SMH_RND_MAX_ITEMS; };

// step 5 of the overlay (imgui's blend, tint alpha 64 / 255) over `u`, from the four taps' colours: the arithmetic of k_hm_overlay
__device__ __forceinline__ uint32_t rnd_blend(uint32_t c00, uint32_t c01, uint32_t c10, uint32_t c11, float fx, float fy, float gy, uint32_t u) {
	const float gx = 1.0f - fx;
	const float A = 64.0f / 255.0f, B = 1.0f - A;
	uint32_t o = 0xFF000000u;
#pragma unroll
	for (uint32_t k = 0; k < 3; ++k) {
		const uint32_t sh = 8u * k;
		const float top = (float)((c00 >> sh) & 255u) * gx + (float)((c01 >> sh) & 255u) * fx;
		const float bot = (float)((c10 >> sh) & 255u) * gx + (float)((c11 >> sh) & 255u) * fx;
		const float c = top * gy + bot * fy;
		const float v = c * A + (float)((u >> sh) & 255u) * B;
		o |= (uint32_t)fminf(v + 0.5f, 255.0f) << sh;
	}
	return o;
}

// floorf(v) as an index clamped to [0, n - 1] (v is finite for every pixel that uses it; the clamp keeps any value in bounds)
__device__ __forceinline__ uint32_t rnd_clamp_index(float fl, float fn, int32_t nm1, int32_t add) {
	const int32_t i = (int32_t)fmaxf(fminf(fl, fn), -1.0f);
	return (uint32_t)min(max(i + add, 0), nm1);
}

__device__ __forceinline__ bool rnd_finite(float v) { return v - v == 0.0f; }

// The colour of a texel from the 16-bit table (k_hm_lut16): byte 0 = the red-or-blue byte (at most one of the two is non-zero: a
// texel above the map's mid height has no blue, one below no red), byte 1 = green; red from vr on, blue below it.  The bytes
// are the 32-bit table's, so the blend sees the same operands.
__device__ __forceinline__ uint32_t rnd_tab_color(const uint16_t *tab, uint32_t v, uint32_t vr) {
	const uint32_t e = tab[v];
	const uint32_t rb = e & 255u;
	return (v >= vr ? rb : rb << 16) | (e & 0xFF00u);
}

// FORM: how the overlay's taps are fetched (the file's header); WAVES: waves per workgroup.  Forms GATHER and STAGE take one tile
// per workgroup (grid: tiles x tiles x frames); form TABLE is persistent -- gridDim.x workgroups of 16 waves copy the heightmap's
// 16-bit colour table (128 KB) into LDS once and then take tiles in turn.
// LAYERS: `y` holds the layers of the call (k_render_map_layers); false: `y` is not read.
template <int FORM, uint32_t WAVES, bool LAYERS>
__device__ __forceinline__ void render_map_body(const Geom g, const RenderRun r, const RenderLayersRun y) {
	constexpr bool STAGE = FORM == SMH_RND_FORM_STAGE, TABLE = FORM == SMH_RND_FORM_TABLE;
	constexpr uint32_t SMH_RND_BAND_ = WAVES, SMH_RND_BANDS = SMH_RND_TH / WAVES;
	extern __shared__ uint32_t s_tex[];                       // STAGE: the colours of r.lds_texels texels of the band's footprint; TABLE: the table
	__shared__ typename RndListOf<LAYERS>::T s_line[RndListOf<LAYERS>::N];
	__shared__ uint32_t s_wave_n[WAVES], s_col[2], s_row[SMH_RND_MAX_BANDS][2];

	const uint32_t tid = threadIdx.x;
	const uint32_t lane_x = tid & 63u, band_row = tid >> 6;
	const uint32_t tiles_x = (r.out_w + SMH_RND_TW - 1u) / SMH_RND_TW, tiles_y = (r.out_h + SMH_RND_TH - 1u) / SMH_RND_TH;
	const uint64_t total = (uint64_t)tiles_x * tiles_y * r.n_frames;
	const uint16_t *s_tab = (const uint16_t *)s_tex;
	uint32_t vr = 0;
	if (TABLE) {
		const uint4 *src = (const uint4 *)r.lut16;
		for (uint32_t i = tid; i < SMH_HM_LUT_ENTRIES / 8u; i += 64u * WAVES) ((uint4 *)s_tex)[i] = src[i];
		vr = r.lut[SMH_HM_LUT_ENTRIES + 2u];
	}
	uint64_t tile = blockIdx.x;                                // (TABLE only: the other forms take the tile of their block index)
	for (;;) {
	uint32_t f = blockIdx.z, bx = blockIdx.x, by = blockIdx.y;
	if (TABLE) {
		if (tile >= total) break;
		__syncthreads();                                       // (the table is in LDS; the previous tile's lists are done with)
		f = (uint32_t)(tile / ((uint64_t)tiles_x * tiles_y));
		const uint32_t t_in = (uint32_t)(tile - (uint64_t)f * tiles_x * tiles_y);
		bx = t_in % tiles_x; by = t_in / tiles_x;
	}
	const uint32_t X0 = bx * SMH_RND_TW + lane_x;              // the lane's pixels: X0 + 64 k
	const uint32_t tile_y = by * SMH_RND_TH;
	uint32_t *out = (uint32_t *)(r.out + (size_t)f * r.out_stride);

	// ---- a closed frame is background everywhere ----
	if (!r.aux[f].open) {
		for (uint32_t bnd = 0; bnd < SMH_RND_BANDS; ++bnd) {
			const uint32_t Y = tile_y + bnd * SMH_RND_BAND_ + band_row;
			if (Y >= r.out_h) continue;
			uint32_t *dst = out + (size_t)Y * r.out_w + X0;
			for (uint32_t k = 0; k < 4u; ++k)
				if (X0 + 64u * k < r.out_w) dst[64u * k] = r.bg;
		}
		if (!TABLE) break;
		tile += gridDim.x;
		continue;
	}

	const smhv_frame_result *res = &r.res[f];
	const bool ovl = (r.flags & SMHV_RENDER_HEIGHTMAP) && res->has_minimap != 0u;
	const uint32_t mm[4] = {res->minimap[0], res->minimap[1], res->minimap[2], res->minimap[3]};
	// the heightmap's rectangle through the viewport: the helper the firing solutions use
	const HmRect q = hm_rect(mm, (r.flags & SMHV_RENDER_BOUNDS_OFFSET) ? SMHV_FIRING_BOUNDS_OFFSET : 0u, r.b0x, r.b0y, r.hm_w, r.hm_h, r.sw, r.sh, r.tx, r.ty);
	const float x0 = q.l, y0 = q.t;
	const float sx = q.r - x0, sy = q.b - y0;
	const float x1 = x0 + sx, y1 = y0 + sy;
	const float fw = (float)r.hm_w, fh = (float)r.hm_h;
	const int32_t wm1 = (int32_t)r.hm_w - 1, hm1 = (int32_t)r.hm_h - 1;
	uint32_t src_w = g.rw, src_h = g.rh;                       // step 1's texture: the ui_map, or the layers' source
	if constexpr (LAYERS) { src_w = y.src_w; src_h = y.src_h; }
	const float mw = (float)src_w, mh = (float)src_h;
	const float qw = r.qr - r.ql, qh = r.qb - r.qt;

	if (tid < 2u + 2u * SMH_RND_BANDS) {
		if (tid < 2u) s_col[tid] = tid == 0u ? 0xFFFFFFFFu : 0u;
		else s_row[(tid - 2u) >> 1][tid & 1u] = (tid & 1u) == 0u ? 0xFFFFFFFFu : 0u;
	}

	// ---- what depends on the column alone ----
	bool mcov[4], ocov[4];
	uint32_t ix[4], ia[4], ib[4];
	float fx[4];
#pragma unroll
	for (uint32_t k = 0; k < 4u; ++k) {
		const float cx = (float)(X0 + 64u * k) + 0.5f;
		const bool inx = X0 + 64u * k < r.out_w;
		mcov[k] = inx && r.ql <= cx && cx < r.qr;
		const float u = ((cx - r.ql) / qw) * mw;
		ix[k] = rnd_clamp_index(floorf(u), mw, (int32_t)src_w - 1, 0);
		ocov[k] = inx && ovl && x0 <= cx && cx < x1;
		const float s = ((cx - x0) / sx) * fw - 0.5f;
		const float i = floorf(s);
		fx[k] = s - i;
		ia[k] = rnd_clamp_index(i, fw, wm1, 0);
		ib[k] = rnd_clamp_index(i, fw, wm1, 1);
	}
	__syncthreads();                                           // (the footprint words are initialised)
	if (STAGE && ovl) {
		// the tile's tap columns and every band's tap rows: minimum and maximum over the covered pixels
		uint32_t lo = 0xFFFFFFFFu, hi = 0u;
#pragma unroll
		for (uint32_t k = 0; k < 4u; ++k)
			if (ocov[k]) { lo = min(lo, min(ia[k], ib[k])); hi = max(hi, max(ia[k], ib[k])); }
		if (lo <= hi && band_row == 0u) { atomicMin(&s_col[0], lo); atomicMax(&s_col[1], hi); }
		if (lane_x == 0u) {
			for (uint32_t bnd = 0; bnd < SMH_RND_BANDS; ++bnd) {
				const uint32_t Y = tile_y + bnd * SMH_RND_BAND_ + band_row;
				const float cy = (float)Y + 0.5f;
				if (Y < r.out_h && y0 <= cy && cy < y1) {
					const float j = floorf(((cy - y0) / sy) * fh - 0.5f);
					const uint32_t ja = rnd_clamp_index(j, fh, hm1, 0), jb = rnd_clamp_index(j, fh, hm1, 1);
					atomicMin(&s_row[bnd][0], min(ja, jb)); atomicMax(&s_row[bnd][1], max(ja, jb));
				}
			}
		}
	}

	// ---- the frame's lines through the viewport, culled against the tile, in order ----
	uint32_t n_lines = 0;
	const smhv_line *lines = nullptr;
	if (r.flags & SMHV_RENDER_MARKERS) {
		if (r.lines) { lines = r.lines; n_lines = min(r.n_lines, SMH_RND_MAX_LINES); }
		else { lines = res->lines; n_lines = min(res->n_lines, (uint32_t)SMHV_MAX_LINES); }
	}
	uint32_t n_list = 0;
	if constexpr (LAYERS) {
		// ---- the layers' list: below-prims, the marker lines, foreground prims, the minimap bounds -- in paint order, culled
		// against the tile and compacted in that order, a workgroup's worth of entries at a time ----
		const bool bounds = (y.flags & SMHV_LAYER_MINIMAP_BOUNDS) && res->has_minimap != 0u;
		const uint32_t e_lines = y.n_below + n_lines, e_fg = e_lines + y.n_fg, n_total = e_fg + (bounds ? 1u : 0u);
		const float cxl = (float)(bx * SMH_RND_TW) + 0.5f, cxh = cxl + (float)(SMH_RND_TW - 1u);
		const float cyl = (float)tile_y + 0.5f, cyh = cyl + (float)(SMH_RND_TH - 1u);
		for (uint32_t chunk = 0; chunk < n_total; chunk += 64u * WAVES) {   // (uniform)
			const uint32_t idx = chunk + tid;
			bool keep = false;
			RndItem it{};
			if (idx < n_total) {
				float p0x, p0y, p1x, p1y;
				uint32_t kind;
				if (idx >= y.n_below && idx < e_lines) {
					const uint32_t li = idx - y.n_below;
					const smhv_line l = lines[li];
					p0x = l.x0 * r.sw + r.tx; p0y = l.y0 * r.sh + r.ty;
					p1x = l.x1 * r.sw + r.tx; p1y = l.y1 * r.sh + r.ty;
					const float fl = (float)(li + 1u) / (float)n_lines;
					it.color = 0xFF000000u | (uint32_t)(uint8_t)((1.0f - fl) * 255.0f + 0.5f) | ((uint32_t)(uint8_t)(fl * 255.0f + 0.5f) << 8);
					kind = SMHV_PRIM_LINE;
				} else if (idx < e_fg) {
					const smhv_render_prim p = y.prims[idx < y.n_below ? idx : idx - n_lines];
					p0x = p.x0 * r.sw + r.tx; p0y = p.y0 * r.sh + r.ty;
					p1x = p.x1 * r.sw + r.tx; p1y = p.y1 * r.sh + r.ty;
					if (p.kind & SMHV_PRIM_SHIFT1) { p0x = p0x + 1.0f; p0y = p0y + 1.0f; p1x = p1x + 1.0f; p1y = p1y + 1.0f; }
					it.color = 0xFF000000u | (uint32_t)p.rgba[0] | ((uint32_t)p.rgba[1] << 8) | ((uint32_t)p.rgba[2] << 16);
					kind = p.kind & 0xFFu;
				} else {                                           // the record's rectangle (left, right, top, bottom), shifted by one
					p0x = ((float)mm[0] * r.sw + r.tx) + 1.0f; p0y = ((float)mm[2] * r.sh + r.ty) + 1.0f;
					p1x = ((float)mm[1] * r.sw + r.tx) + 1.0f; p1y = ((float)mm[3] * r.sh + r.ty) + 1.0f;
					it.color = 0xFF00FF00u;
					kind = SMHV_PRIM_RECT;
				}
				it.kind = kind;
				const float big = fmaxf(fmaxf(fmaxf(fabsf(p0x), fabsf(p0y)), fmaxf(fabsf(p1x), fabsf(p1y))), fmaxf(cxh, cyh));
				const bool fin = rnd_finite(p0x) && rnd_finite(p0y) && rnd_finite(p1x) && rnd_finite(p1y);
				if (kind == SMHV_PRIM_RECT) {
					// fminf / fmaxf return the other operand for a NaN one.  The test compares the centres with the corners
					// themselves, so the outer box alone decides; it is grown by the rounding of coordinates of this size all the same
					it.a = fminf(p0x, p1x); it.b = fminf(p0y, p1y); it.c = fmaxf(p0x, p1x); it.d = fmaxf(p0y, p1y);
					const float m = 4e-6f * big;
					const bool away = it.c + m < cxl || it.a - m > cxh || it.d + m < cyl || it.b - m > cyh;
					keep = !fin || !away;
				} else {
					it.a = p0x; it.b = p0y;
					it.c = p1x - p0x; it.d = p1y - p0y;
					it.len2 = it.c * it.c + it.d * it.d;
					if (it.len2 > 0.0f) {                          // (the cull of the lines below, word for word)
						const float m = 2.0f + 4e-6f * big;
						const bool away = fmaxf(p0x, p1x) + m < cxl || fminf(p0x, p1x) - m > cxh || fmaxf(p0y, p1y) + m < cyl || fminf(p0y, p1y) - m > cyh;
						keep = !(fin && rnd_finite(it.len2)) || !away;
					}
				}
			}
			const unsigned long long bal = __ballot(keep);
			const uint32_t wave = tid >> 6, lane = tid & 63u;
			if (lane == 0u) s_wave_n[wave] = (uint32_t)__popcll(bal);
			__syncthreads();
			uint32_t base = n_list;
			for (uint32_t w = 0; w < WAVES; ++w) {
				if (w < wave) base += s_wave_n[w];
				n_list += s_wave_n[w];
			}
			if (keep) s_line[base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = it;
			__syncthreads();                                       // (the next chunk rewrites the waves' counts)
		}
	} else
	if (n_lines) {                                             // (uniform)
		bool keep = false;
		RndLine ln{};
		if (tid < n_lines) {
			const smhv_line l = lines[tid];
			const float p0x = l.x0 * r.sw + r.tx, p0y = l.y0 * r.sh + r.ty;
			const float p1x = l.x1 * r.sw + r.tx, p1y = l.y1 * r.sh + r.ty;
			ln.px = p0x; ln.py = p0y;
			ln.dx = p1x - p0x; ln.dy = p1y - p0y;
			ln.len2 = ln.dx * ln.dx + ln.dy * ln.dy;
			const float fl = (float)(tid + 1u) / (float)n_lines;
			ln.color = 0xFF000000u | (uint32_t)(uint8_t)((1.0f - fl) * 255.0f + 0.5f) | ((uint32_t)(uint8_t)(fl * 255.0f + 0.5f) << 8);
			if (ln.len2 > 0.0f) {
				// A pixel is painted when its centre is within 1.0 of the segment as f32 arithmetic sees it.  The cull keeps every
				// line whose bounding box, grown by 2 px plus the rounding of coordinates of this size, touches the tile's pixel
				// centres, and every line with a coordinate that is not finite.
				const float cxl = (float)(bx * SMH_RND_TW) + 0.5f, cxh = cxl + (float)(SMH_RND_TW - 1u);
				const float cyl = (float)tile_y + 0.5f, cyh = cyl + (float)(SMH_RND_TH - 1u);
				const float big = fmaxf(fmaxf(fmaxf(fabsf(p0x), fabsf(p0y)), fmaxf(fabsf(p1x), fabsf(p1y))), fmaxf(cxh, cyh));
				const float m = 2.0f + 4e-6f * big;
				const bool fin = rnd_finite(p0x) && rnd_finite(p0y) && rnd_finite(p1x) && rnd_finite(p1y) && rnd_finite(ln.len2);
				const bool away = fmaxf(p0x, p1x) + m < cxl || fminf(p0x, p1x) - m > cxh || fmaxf(p0y, p1y) + m < cyl || fminf(p0y, p1y) - m > cyh;
				keep = !fin || !away;
			}
		}
		const unsigned long long bal = __ballot(keep);
		const uint32_t wave = tid >> 6, lane = tid & 63u;
		if (lane == 0u) s_wave_n[wave] = (uint32_t)__popcll(bal);
		__syncthreads();
		uint32_t base = 0;
		for (uint32_t w = 0; w < WAVES; ++w) {
			if (w < wave) base += s_wave_n[w];
			n_list += s_wave_n[w];
		}
		if (keep) s_line[base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = ln;
	}
	__syncthreads();

	uint32_t c_lo = 0, c_w = 0;
	if (STAGE && ovl && s_col[0] <= s_col[1]) { c_lo = s_col[0]; c_w = s_col[1] - c_lo + 1u; }

	for (uint32_t bnd = 0; bnd < SMH_RND_BANDS; ++bnd) {
		// ---- <true>: the band's footprint into LDS (uniform decisions) ----
		bool staged = false;
		uint32_t r_lo = 0;
		if (STAGE) {
			const uint32_t lo = s_row[bnd][0], hi = s_row[bnd][1];
			if (c_w != 0u && lo <= hi) {
				const uint32_t r_h = hi - lo + 1u;
				if ((uint64_t)c_w * r_h <= (uint64_t)r.lds_texels) {
					staged = true; r_lo = lo;
					const uint32_t wave = tid >> 6, lane = tid & 63u;
					for (uint32_t rr = wave; rr < r_h; rr += WAVES) {
						const uint16_t *src = r.hm + (size_t)(lo + rr) * r.hm_w + c_lo;
						for (uint32_t cc = lane; cc < c_w; cc += 64u) s_tex[rr * c_w + cc] = r.lut[src[cc]];
					}
				}
			}
			__syncthreads();
		}
		const uint32_t Y = tile_y + bnd * SMH_RND_BAND_ + band_row;
		if (Y < r.out_h && X0 < r.out_w) {                       // (wave-uniform in Y; lanes right of the window sit out)
			const float cy = (float)Y + 0.5f;
			// step 1: the map quad's texel row
			const bool mrow = r.qt <= cy && cy < r.qb;
			const uint32_t iy = rnd_clamp_index(floorf(((cy - r.qt) / qh) * mh), mh, (int32_t)src_h - 1, 0);
			uint32_t o[4];
			bool other = false;
			if constexpr (LAYERS) other = y.src_mode != SMH_RND_SRC_UI;
			if (other) {            // (uniform) a debug view is the quad's texture
#pragma unroll
				for (uint32_t k = 0; k < 4u; ++k) o[k] = r.bg;
				if (mrow) {
					if (y.src_mode == SMH_RND_SRC_GRAY) {              // one byte per pixel, 64 neighbouring bytes per load
						const uint8_t *row = y.src + (size_t)f * y.src_stride + (size_t)iy * y.src_pitch + y.src_xoff;
#pragma unroll
						for (uint32_t k = 0; k < 4u; ++k)
							if (mcov[k]) o[k] = (uint32_t)row[ix[k]] * 0x00010101u | 0xFF000000u;
					} else if (y.src_mode == SMH_RND_SRC_RGBA) {        // the per-call path: smhv_get_debug_view's image, tightly packed
						const uint32_t *row = (const uint32_t *)(y.src + (size_t)iy * y.src_pitch);
#pragma unroll
						for (uint32_t k = 0; k < 4u; ++k)
							if (mcov[k]) o[k] = row[ix[k]] | 0xFF000000u;
					} else {                                           // the colour ui_map: isolated (LSD_PREPROCESS) or its bottom right quarter
						const bool crop = y.src_mode == SMH_RND_SRC_CROPPED;
						const uint32_t oy = crop ? g.rh / 2u : 0u, ox = crop ? g.rw / 2u : 0u;
						const uint32_t *row = (const uint32_t *)(r.ui + (size_t)f * g.ui_stride + (size_t)(iy + oy) * g.ui_pitch) + g.m_xoff + ox;
#pragma unroll
						for (uint32_t k = 0; k < 4u; ++k)
							if (mcov[k]) {
								const uint32_t p = row[ix[k]];
								o[k] = (crop || is_marker(p & 255u, (p >> 8) & 255u, (p >> 16) & 255u)) ? (p | 0xFF000000u) : 0xFF000000u;
							}
					}
				}
			} else {
			const uint32_t *src = (const uint32_t *)(r.ui + (size_t)f * g.ui_stride + (size_t)iy * g.ui_pitch) + g.m_xoff;
#pragma unroll
			for (uint32_t k = 0; k < 4u; ++k) o[k] = (mrow && mcov[k]) ? (src[ix[k]] | 0xFF000000u) : r.bg;
			}
			// step 2: the overlay
			if (ovl && y0 <= cy && cy < y1) {
				const float t = ((cy - y0) / sy) * fh - 0.5f;
				const float j = floorf(t);
				const float fy = t - j, gy = 1.0f - fy;
				const uint32_t ja = rnd_clamp_index(j, fh, hm1, 0), jb = rnd_clamp_index(j, fh, hm1, 1);
				uint32_t tp[4][4];
				if (STAGE && staged) {
					const uint32_t *ra = s_tex + (ja - r_lo) * c_w, *rb = s_tex + (jb - r_lo) * c_w;
#pragma unroll
					for (uint32_t k = 0; k < 4u; ++k)
						if (ocov[k]) { tp[k][0] = ra[ia[k] - c_lo]; tp[k][1] = ra[ib[k] - c_lo]; tp[k][2] = rb[ia[k] - c_lo]; tp[k][3] = rb[ib[k] - c_lo]; }
				} else {
					const uint16_t *ra = r.hm + (size_t)ja * r.hm_w, *rb = r.hm + (size_t)jb * r.hm_w;
#pragma unroll
					for (uint32_t k = 0; k < 4u; ++k)
						if (ocov[k]) { tp[k][0] = ra[ia[k]]; tp[k][1] = ra[ib[k]]; tp[k][2] = rb[ia[k]]; tp[k][3] = rb[ib[k]]; }
					if (TABLE) {
#pragma unroll
						for (uint32_t k = 0; k < 4u; ++k)
							if (ocov[k]) {
#pragma unroll
								for (uint32_t q4 = 0; q4 < 4u; ++q4) tp[k][q4] = rnd_tab_color(s_tab, tp[k][q4], vr);
							}
					} else {
#pragma unroll
						for (uint32_t k = 0; k < 4u; ++k)
							if (ocov[k]) { tp[k][0] = r.lut[tp[k][0]]; tp[k][1] = r.lut[tp[k][1]]; tp[k][2] = r.lut[tp[k][2]]; tp[k][3] = r.lut[tp[k][3]]; }
					}
				}
#pragma unroll
				for (uint32_t k = 0; k < 4u; ++k)
					if (ocov[k]) o[k] = rnd_blend(tp[k][0], tp[k][1], tp[k][2], tp[k][3], fx[k], fy, gy, o[k]);
			}
			// step 3: the lines that reach this tile, last first: the first hit is the line painted last
			if (n_list) {
				bool done[4] = {false, false, false, false};
				for (uint32_t li = n_list; li-- > 0u;) {
					if constexpr (LAYERS) {
						const RndItem it = s_line[li];
						if (it.kind == SMHV_PRIM_RECT) {               // (uniform) a 1 px frame: the outer box without the inner one
							const bool yin = it.b <= cy && cy < it.d, yinner = it.b + 1.0f <= cy && cy < it.d - 1.0f;
#pragma unroll
							for (uint32_t k = 0; k < 4u; ++k) {
								const float cx = (float)(X0 + 64u * k) + 0.5f;
								const bool in = yin && it.a <= cx && cx < it.c;
								const bool inner = yinner && it.a + 1.0f <= cx && cx < it.c - 1.0f;
								if (!done[k] && in && !inner) { o[k] = it.color; done[k] = true; }
							}
						} else {
							const float ay = cy - it.b;
#pragma unroll
							for (uint32_t k = 0; k < 4u; ++k) {
								const float ax = ((float)(X0 + 64u * k) + 0.5f) - it.a;
								const float t = ax * it.c + ay * it.d;
								const float c = ax * it.d - ay * it.c;
								if (!done[k] && 0.0f <= t && t <= it.len2 && c * c <= it.len2) { o[k] = it.color; done[k] = true; }
							}
						}
					} else {
					const RndLine ln = s_line[li];
					const float ay = cy - ln.py;
#pragma unroll
					for (uint32_t k = 0; k < 4u; ++k) {
						const float ax = ((float)(X0 + 64u * k) + 0.5f) - ln.px;
						const float t = ax * ln.dx + ay * ln.dy;
						const float c = ax * ln.dy - ay * ln.dx;
						if (!done[k] && 0.0f <= t && t <= ln.len2 && c * c <= ln.len2) { o[k] = ln.color; done[k] = true; }
					}
					}
				}
			}
			uint32_t *dst = out + (size_t)Y * r.out_w + X0;
#pragma unroll
			for (uint32_t k = 0; k < 4u; ++k)
				if (X0 + 64u * k < r.out_w) dst[64u * k] = o[k];
		}
		if (STAGE) __syncthreads();                            // (the next band overwrites the footprint)
	}
	if (!TABLE) break;
	tile += gridDim.x;
	}
}

template <int FORM, uint32_t WAVES>
__global__ void __launch_bounds__(64 * WAVES) k_render_map(Geom g, RenderRun r) {
	render_map_body<FORM, WAVES, false>(g, r, RenderLayersRun{});
}
template <int FORM, uint32_t WAVES>
__global__ void __launch_bounds__(64 * WAVES) k_render_map_layers(Geom g, RenderRun r, RenderLayersRun y) {
	render_map_body<FORM, WAVES, true>(g, r, y);
}

// The 16-bit colour table of a heightmap from its 32-bit one, and vr = the lowest texel value whose colour has red (65,536: none).
// Red rises and blue falls with the value, and no colour has both, so (value >= vr) says which of the two the shared byte is.
__global__ void __launch_bounds__(256) k_hm_lut16(const uint32_t *__restrict__ lut, uint16_t *__restrict__ lut16, uint32_t *vr) {
	const uint32_t v = blockIdx.x * 256u + threadIdx.x;
	const uint32_t c = lut[v];
	const uint32_t red = c & 255u, green = (c >> 8) & 255u, blue = (c >> 16) & 255u;
	lut16[v] = (uint16_t)((red | blue) | (green << 8));
	if (red) atomicMin(vr, v);
}

hipError_t launch_heightmap_lut16(const uint32_t *lut, uint16_t *lut16, uint32_t *vr, hipStream_t s) {
	static const uint32_t none = SMH_HM_LUT_ENTRIES;
	hipError_t e = hipMemcpyAsync(vr, &none, sizeof none, hipMemcpyHostToDevice, s);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_hm_lut16, dim3(SMH_HM_LUT_ENTRIES / 256u), dim3(256), 0, s, lut, lut16, vr);
	return hipGetLastError();
}

// The form and its LDS for a call (host).  The staged form's LDS is the texel footprint of one band of a tile, from the
// texels-per-pixel ratios of the viewport with the minimap rectangle = the whole ROI.  A real frame's rectangle is a part of the
// ROI (and SMHV_RENDER_BOUNDS_OFFSET shrinks it further), which RAISES the ratios: the estimate is a lower bound, so the LDS is
// given half as much again, and a band whose footprint still exceeds it gathers (correct, slower).
// SMH_RND_STAGE_RATIO: texels per pixel up to which the staged form is taken, above it the table form.  tools/render_cost.py
// measures the forms side by side (profiles/render_cost.json): the table form is the fastest at every ratio measured, 0.42 to 27
// texels per pixel, so the ratio is 0 and the rule always takes the table; the other two stay for comparison and for the tests.  SMH_RND_STAGE_MAX_BYTES: with the line list two workgroups still
// share a CU's LDS.
#define SMH_RND_STAGE_MAX_BYTES 49152u
#define SMH_RND_STAGE_RATIO 0.0f
static uint32_t g_render_form = 0;      // smhv_debug_render_form: 0 = the rule, 1 = gathers, 2 = LDS staging, 3 = the table in LDS
void render_set_form(uint32_t form) { g_render_form = form <= 3u ? form : 0u; }
float render_switch_ratio() { return SMH_RND_STAGE_RATIO; }

uint32_t render_rule(const Geom &g, const RenderRun &r, uint32_t *texels, float *ratio) {
	const double px_w = (double)g.rw * fabs((double)r.sw), px_h = (double)g.rh * fabs((double)r.sh);
	double rx = px_w > 0.0 ? (double)r.hm_w / px_w : 1e30, ry = px_h > 0.0 ? (double)r.hm_h / px_h : 1e30;
	if (!(rx == rx) || !(ry == ry)) rx = ry = 1e30;
	const double ra = fmin(rx * ry, 1e30);
	if (ratio) *ratio = (float)ra;
	const double cols = fmin(ceil((double)SMH_RND_TW * rx) + 3.0, (double)r.hm_w), rows = fmin(ceil((double)SMH_RND_BAND * ry) + 3.0, (double)r.hm_h);
	const double want = cols * rows;
	const bool fits = want * 4.0 <= (double)SMH_RND_STAGE_MAX_BYTES;
	const double room = fmin(want * 1.5, (double)(SMH_RND_STAGE_MAX_BYTES / 4u));
	if (texels) *texels = fits ? (room < 1024.0 ? 1024u : (uint32_t)room) : SMH_RND_STAGE_MAX_BYTES / 4u;
	return (fits && ra <= (double)SMH_RND_STAGE_RATIO) ? 2u : 3u;
}

// y == nullptr: the kernels without layers (k_render_map); else k_render_map_layers of the same form
static hipError_t launch_render(const Geom &g, const RenderRun &run, const RenderLayersRun *y, uint32_t n, hipStream_t s) {
	RenderRun r = run;
	const uint32_t tiles_x = (r.out_w + SMH_RND_TW - 1u) / SMH_RND_TW, tiles_y = (r.out_h + SMH_RND_TH - 1u) / SMH_RND_TH;
	const dim3 grid(tiles_x, tiles_y, n);
	r.lds_texels = 0;
	r.n_frames = n;
	uint32_t form = 1u;
	if ((r.flags & SMHV_RENDER_HEIGHTMAP) && r.hm) {
		uint32_t texels = 0;
		form = render_rule(g, r, &texels, nullptr);
		if (g_render_form) form = g_render_form;
		if (form == 2u) r.lds_texels = texels;
	}
	if (form == 3u) {
		// persistent: one workgroup of 16 waves per CU (the table takes 128 of its 160 KB of LDS), fewer when there are fewer tiles
		static bool attr_set[2] = {false, false};
		const size_t tab_bytes = (size_t)SMH_HM_LUT_ENTRIES * 2u;
		const void *fn = y ? (const void *)k_render_map_layers<SMH_RND_FORM_TABLE, SMH_RND_TABLE_WAVES> : (const void *)k_render_map<SMH_RND_FORM_TABLE, SMH_RND_TABLE_WAVES>;
		if (!attr_set[y ? 1 : 0]) {
			hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tab_bytes);
			if (e != hipSuccess) return e;
			attr_set[y ? 1 : 0] = true;
		}
		int dev = 0, cus = 0;
		hipError_t e = hipGetDevice(&dev);
		if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
		if (e != hipSuccess) return e;
		const uint64_t total = (uint64_t)tiles_x * tiles_y * n;
		const uint32_t wgs = (uint32_t)(total < (uint64_t)cus ? total : (uint64_t)cus);
		if (y) hipLaunchKernelGGL((k_render_map_layers<SMH_RND_FORM_TABLE, SMH_RND_TABLE_WAVES>), dim3(wgs), dim3(64u * SMH_RND_TABLE_WAVES), tab_bytes, s, g, r, *y);
		else hipLaunchKernelGGL((k_render_map<SMH_RND_FORM_TABLE, SMH_RND_TABLE_WAVES>), dim3(wgs), dim3(64u * SMH_RND_TABLE_WAVES), tab_bytes, s, g, r);
	} else if (form == 2u) {
		if (y) hipLaunchKernelGGL((k_render_map_layers<SMH_RND_FORM_STAGE, 4u>), grid, dim3(256), (size_t)r.lds_texels * 4u, s, g, r, *y);
		else hipLaunchKernelGGL((k_render_map<SMH_RND_FORM_STAGE, 4u>), grid, dim3(256), (size_t)r.lds_texels * 4u, s, g, r);
	} else {
		if (y) hipLaunchKernelGGL((k_render_map_layers<SMH_RND_FORM_GATHER, 4u>), grid, dim3(256), 0, s, g, r, *y);
		else hipLaunchKernelGGL((k_render_map<SMH_RND_FORM_GATHER, 4u>), grid, dim3(256), 0, s, g, r);
	}
	return hipGetLastError();
}

hipError_t launch_render_map(const Geom &g, const RenderRun &run, uint32_t n, hipStream_t s) { return launch_render(g, run, nullptr, n, s); }
hipError_t launch_render_map_layers(const Geom &g, const RenderRun &run, const RenderLayersRun &y, uint32_t n, hipStream_t s) { return launch_render(g, run, &y, n, s); }

}  // namespace smh
