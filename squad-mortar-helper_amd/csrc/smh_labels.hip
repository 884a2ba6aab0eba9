// smh_labels.hip -- the marker labels of the map view: range, mils, bearings and altitude as text (gfx950, wave64).
//   k_label_plan   src/ui/markers.rs:93-211: the firing solution of every labelled line (firing_line, smh_firing.h), its strings,
//                  their layout and placement -> the label slab (smhv_label_result per frame) and a cull entry per slot
//   k_label_draw   the pixel rule over a finished image of the map view (the render slab)
//
// The semantics are spelt out in include/smh_vision_hip.h ("map view: labels"); every operation below that feeds a slot or a pixel
// is one of its operations, in its order, unfused (-ffp-contract=off, IEEE division and square root).
//
// k_label_plan: one workgroup per frame, one lane per slot.  A string is built in two 64-bit registers (a character is a shift and
// an OR at a computed position), a number from its last digit backwards: there is no per-lane array and no formatted print.
// k_label_draw: output-driven.  A workgroup of four waves takes a tile of SMH_LBL_TW x SMH_LBL_TH = 64 x 32 pixels of one frame: a
// wave a row at a time, a lane a column, so a row's stores are 256 contiguous bytes.  A label at S = 2 is about 140 x 72 px: a
// tile of that order keeps the pixels tested for nothing few, and almost every tile of a window meets no label at all -- it reads
// one word (n_labels) and the frame's cull entries (16 bytes per slot, written by the plan) and leaves before it touches the
// image or the slots.  The survivors are compacted in slot order into an LDS list (ballot and prefix, as the render kernel's
// lines); a lane walks the list from its end and takes the first hit: the label painted last.  Only painted pixels are stored.
#include "smh_device.h"
#include "smh_firing.h"
#include "smh_font5x7.h"

namespace smh {

#define SMH_LBL_TW 64u
#define SMH_LBL_TH 32u
#define SMH_LBL_WAVES 4u
#define SMH_LBL_RUNS 6u
static_assert(sizeof(smhv_label_line) == 20 && sizeof(smhv_label_run) == 24 && sizeof(smhv_label) == 216, "the slot's layout is public");
static_assert(sizeof(smhv_label_result) == 8 + 216 * SMH_LBL_SLOTS, "the slab's layout is public");
static_assert(SMH_LBL_SLOTS <= 128u, "k_label_plan: a lane per slot; k_label_draw: the cull takes two waves");

__constant__ uint8_t c_font[SMH_FONT_GLYPHS][SMH_FONT_ROWS] = SMH_FONT5X7_TABLE;

// ---- a string of up to 16 Latin-1 bytes in registers ----
struct LblText { uint64_t lo, hi; uint32_t n; };
__device__ __forceinline__ void lbl_set(LblText &t, uint32_t pos, uint32_t c) {
	const uint64_t v = (uint64_t)c << ((pos & 7u) * 8u);
	if (pos < 8u) t.lo |= v;
	else t.hi |= v;
}
__device__ __forceinline__ void lbl_ch(LblText &t, uint32_t c) { lbl_set(t, t.n, c); ++t.n; }
// an unsigned decimal, from the last digit backwards
__device__ __forceinline__ void lbl_num(LblText &t, uint32_t v) {
	const uint32_t nd = 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) +
	                    (v >= 1000000000u);
	for (uint32_t i = 0; i < nd; ++i) {
		lbl_set(t, t.n + nd - 1u - i, 48u + v % 10u);
		v /= 10u;
	}
	t.n += nd;
}
// {:.0} of a non-negative f64: rint (ties to even) as an unsigned decimal
__device__ __forceinline__ uint32_t lbl_rint(double v) {
	const double r = rint(v);
	return r > 0.0 ? (r < 4294967295.0 ? (uint32_t)r : 0xFFFFFFFFu) : 0u;
}
// "RANGE!" when the mils are NaN, else "{rint} mil"
__device__ __forceinline__ void lbl_mil(LblText &t, double m) {
	if (!(m == m)) {
		lbl_ch(t, 'R'); lbl_ch(t, 'A'); lbl_ch(t, 'N'); lbl_ch(t, 'G'); lbl_ch(t, 'E'); lbl_ch(t, '!');
	} else {
		lbl_num(t, lbl_rint(m));
		lbl_ch(t, ' '); lbl_ch(t, 'm'); lbl_ch(t, 'i'); lbl_ch(t, 'l');
	}
}
// "{bearing}deg", with `arrow` ('>' or '<', 0: none) "-> " / "<- " in front
__device__ __forceinline__ void lbl_bearing(LblText &t, uint32_t arrow, float b) {
	if (arrow == '>') { lbl_ch(t, '-'); lbl_ch(t, '>'); lbl_ch(t, ' '); }
	if (arrow == '<') { lbl_ch(t, '<'); lbl_ch(t, '-'); lbl_ch(t, ' '); }
	lbl_num(t, (uint32_t)b);
	lbl_ch(t, 0xB0u);
}
__device__ __forceinline__ void lbl_store_run(smhv_label_run *run, int32_t x2, int32_t y2, const LblText &t) {
	uint32_t *w = (uint32_t *)run;
	w[0] = ((uint32_t)x2 & 0xFFFFu) | ((uint32_t)y2 << 16);
	w[1] = t.n;
	w[2] = (uint32_t)t.lo; w[3] = (uint32_t)(t.lo >> 32); w[4] = (uint32_t)t.hi; w[5] = (uint32_t)(t.hi >> 32);
}
// the farthest corner of a run from the label's origin, squared, in half font units
__device__ __forceinline__ uint32_t lbl_reach2(int32_t x2, int32_t y2, uint32_t n) {
	const int32_t xb = x2 + 12 * (int32_t)n, yb = y2 + 18;
	return (uint32_t)max(x2 * x2, xb * xb) + (uint32_t)max(y2 * y2, yb * yb);
}
__device__ __forceinline__ bool lbl_finite(float v) { return v - v == 0.0f; }

__global__ void __launch_bounds__(128) k_label_plan(LabelRun r) {
	const uint32_t f = blockIdx.x, lane = threadIdx.x;
	if (lane >= SMH_LBL_SLOTS) return;
	smhv_label_result *out = &r.out[f];
	LabelCull *cull = r.cull + (size_t)f * SMH_LBL_SLOTS;
	const smhv_frame_result *res = r.per_call ? r.res : &r.res[f];
	uint32_t n_det = 0;
	if (r.detected) n_det = r.per_call ? r.n_lines : min(res->n_lines, (uint32_t)SMHV_MAX_LINES);
	const uint32_t n_slots = r.aux[f].open ? r.n_extra + n_det : 0u;
	if (lane == 0u) { out->n_labels = n_slots; out->reserved = 0u; }
	smhv_label *slot = &out->label[lane];
	uint32_t *sw = (uint32_t *)slot;
	LabelCull cl{0.0f, 0.0f, 0.0f, 0u};
	if (lane >= n_slots) {
		for (uint32_t k = 0; k < sizeof(smhv_label) / 4u; ++k) sw[k] = 0u;
		cull[lane] = cl;
		return;
	}
	const bool has_mpx = (r.per_call ? r.has_mpx : res->has_mpx) != 0u;
	const double mpx = r.per_call ? r.mpx : res->mpx;
	const uint32_t mm[4] = {res->minimap[0], res->minimap[1], res->minimap[2], res->minimap[3]};
	smhv_line ln;
	uint32_t color;
	double met = 0.0;
	bool own_meters = true;                                      // Marker::new's meters from the line itself
	if (lane < r.n_extra) {
		const smhv_label_line e = r.extra[lane];
		ln = e.line;
		color = (uint32_t)e.rgba[0] | ((uint32_t)e.rgba[1] << 8) | ((uint32_t)e.rgba[2] << 16) | 0xFF000000u;
	} else {
		const uint32_t j = lane - r.n_extra;
		if (r.per_call) ln = r.lines[j];
		else { ln = res->lines[j]; met = res->meters[j]; own_meters = false; }
		const float fl = (float)(j + 1u) / (float)n_det;
		color = 0xFF000000u | (uint32_t)(uint8_t)((1.0f - fl) * 255.0f + 0.5f) | ((uint32_t)(uint8_t)(fl * 255.0f + 0.5f) << 8);
	}
	if (own_meters) {
		const double ax = (double)ln.x0 - (double)ln.x1, ay = (double)ln.y0 - (double)ln.y1;
		met = has_mpx ? sqrt(ax * ax + ay * ay) * mpx : 0.0;
	}
	const smhv_firing o = firing_line(r.fr, res->has_minimap != 0u, mm, ln, has_mpx, met);

	const float p0x = ln.x0 * r.fr.sw + r.fr.tx, p0y = ln.y0 * r.fr.sh + r.fr.ty;
	const float p1x = ln.x1 * r.fr.sw + r.fr.tx, p1y = ln.y1 * r.fr.sh + r.fr.ty;
	const float dx = p0x - p1x, dy = p0y - p1y;
	const float len2 = dx * dx + dy * dy;
	const bool label = o.source != SMHV_FIRING_NONE && lbl_finite(p0x) && lbl_finite(p0y) && lbl_finite(p1x) && lbl_finite(p1y) && !(len2 == 0.0f) &&
	                   o.meters < 999999.5;

	LblText t0{0, 0, 0}, t1{0, 0, 0}, t2{0, 0, 0}, t3{0, 0, 0}, t4{0, 0, 0}, t5{0, 0, 0};
	int32_t x0 = 0, x1 = 0, x2 = 0, x3 = 0, x4 = 0, x5 = 0, y2 = 0, y3 = 0, y4 = 0, y5 = 0;
	uint32_t n_runs = 0;
	float mx = 0.0f, my = 0.0f, ex = 0.0f, ey = 0.0f;
	if (label) {
		lbl_num(t0, lbl_rint(o.meters));
		lbl_ch(t0, 'm');
		if (o.source == SMHV_FIRING_SCALES) {
			n_runs = 4u;
			lbl_mil(t1, o.mils[0]);
			const bool right = dx >= 0.0f;
			lbl_bearing(t2, '>', right ? o.bearing[1] : o.bearing[0]);
			lbl_bearing(t3, '<', right ? o.bearing[0] : o.bearing[1]);
			const int32_t w0 = 6 * (int32_t)t0.n, w1 = 6 * (int32_t)t1.n, w2 = 6 * (int32_t)t2.n, w3 = 6 * (int32_t)t3.n;
			const int32_t W2 = max(w0, w1), W4 = max(W2, max(w2, w3));
			x0 = -W2 + (W4 - w0); x1 = -W2 + (W4 - w1); x2 = -W2 + (W4 - w2); x3 = -W2 + (W4 - w3);
			y2 = 36; y3 = 54;
		} else {
			n_runs = 6u;
			// A = |alt_delta as i32|: truncating, saturating, NaN -> 0
			const double at = trunc(o.alt_delta);
			uint32_t A;
			if (!(at == at)) A = 0u;
			else if (at >= 2147483647.0) A = 2147483647u;
			else if (at <= -2147483648.0) A = 2147483648u;
			else A = (uint32_t)abs((int32_t)at);
			lbl_ch(t1, 0xB1u);
			lbl_num(t1, A);
			lbl_ch(t1, 'm'); lbl_ch(t1, ' '); lbl_ch(t1, 'a'); lbl_ch(t1, 'l'); lbl_ch(t1, 't');
			const bool fwd = dx > 0.0f || (dx == 0.0f && dy < 0.0f);
			const uint32_t a = fwd ? 0u : 1u, b = 1u - a;
			lbl_ch(t2, '<'); lbl_ch(t2, '-'); lbl_ch(t2, ' ');
			lbl_mil(t2, a ? o.mils[1] : o.mils[0]);
			lbl_bearing(t3, 0u, a ? o.bearing[1] : o.bearing[0]);
			lbl_mil(t4, b ? o.mils[1] : o.mils[0]);
			lbl_ch(t4, ' '); lbl_ch(t4, '-'); lbl_ch(t4, '>');
			lbl_bearing(t5, 0u, b ? o.bearing[1] : o.bearing[0]);
			const int32_t w2 = 6 * (int32_t)t2.n, w3 = 6 * (int32_t)t3.n, w4 = 6 * (int32_t)t4.n, w5 = 6 * (int32_t)t5.n;
			const int32_t Wf = max(w2, w3), Wb = max(w4, w5), G = 5;
			x0 = -6 * (int32_t)t0.n; x1 = -6 * (int32_t)t1.n;
			const int32_t xb = -(Wf + Wb + G);
			x2 = xb + 2 * (Wf - w2); x3 = xb + 2 * (Wf - w3);
			x4 = x5 = xb + 2 * (G + Wf);
			y2 = 36; y3 = 54; y4 = 36; y5 = 54;
		}
		mx = (p0x + p1x) / 2.0f; my = (p0y + p1y) / 2.0f;
		const float len = sqrtf(len2);
		const float s = dx > 0.0f ? 1.0f : -1.0f;
		ex = (s * dx) / len; ey = (s * dy) / len;
		// the cull's circle about M: the farthest corner of a run, through the scale of e as it came out (1 but for rounding;
		// anything else when len2 left f32's range -- then, or when a value is not finite, every tile keeps the label)
		uint32_t reach2 = max(max(lbl_reach2(x0, 0, t0.n), lbl_reach2(x1, 18, t1.n)), max(lbl_reach2(x2, y2, t2.n), lbl_reach2(x3, y3, t3.n)));
		if (n_runs == 6u) reach2 = max(reach2, max(lbl_reach2(x4, y4, t4.n), lbl_reach2(x5, y5, t5.n)));
		const float en = sqrtf(ex * ex + ey * ey);
		cl.mx = mx; cl.my = my;
		if (lbl_finite(mx) && lbl_finite(my) && en > 0.5f && en < 2.0f) {
			cl.rad = ((sqrtf((float)reach2) * 0.5f * (float)r.scale) / en) * 1.0001f + 2.0f;
			cl.live = 1u;
		} else
			cl.live = 2u;
	}
	slot->firing = o;
	slot->mid[0] = mx; slot->mid[1] = my;
	slot->dir[0] = ex; slot->dir[1] = ey;
	sw[16] = color;
	slot->n_runs = n_runs;
	lbl_store_run(&slot->run[0], x0, 0, t0);
	lbl_store_run(&slot->run[1], x1, n_runs ? 18 : 0, t1);
	lbl_store_run(&slot->run[2], x2, y2, t2);
	lbl_store_run(&slot->run[3], x3, y3, t3);
	lbl_store_run(&slot->run[4], x4, y4, t4);
	lbl_store_run(&slot->run[5], x5, y5, t5);
	cull[lane] = cl;
}

// a survivor of the cull as the pixel loop reads it: offsets as floats ((float)x2 * 0.5f is exact), characters as glyph numbers
struct LblItem {
	float mx, my, ex, ey;
	uint32_t color, n_runs;
	float ox[SMH_LBL_RUNS], oy[SMH_LBL_RUNS], wd[SMH_LBL_RUNS];      // wd = (float)(6 * chars)
	uint8_t glyph[SMH_LBL_RUNS][16];
};

__global__ void __launch_bounds__(64 * SMH_LBL_WAVES) k_label_draw(LabelRun r) {
	__shared__ LblItem s_item[SMH_LBL_SLOTS];
	__shared__ uint8_t s_font[SMH_FONT_GLYPHS * SMH_FONT_ROWS + 3];
	__shared__ uint32_t s_wave_n[SMH_LBL_WAVES], s_slot[SMH_LBL_SLOTS];

	const uint32_t f = blockIdx.z, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
	const smhv_label_result *lab = &r.out[f];
	const uint32_t n_slots = min(lab->n_labels, SMH_LBL_SLOTS);  // (uniform)
	if (n_slots == 0u) return;
	const uint32_t tile_x = blockIdx.x * SMH_LBL_TW, tile_y = blockIdx.y * SMH_LBL_TH;

	// ---- the frame's slots against the tile: the circle about M, grown by the rounding of coordinates of this size ----
	bool keep = false;
	if (tid < n_slots) {
		const LabelCull c = r.cull[(size_t)f * SMH_LBL_SLOTS + tid];
		if (c.live == 2u) keep = true;
		else if (c.live == 1u) {
			const float cxl = (float)tile_x + 0.5f, cxh = cxl + (float)(SMH_LBL_TW - 1u);
			const float cyl = (float)tile_y + 0.5f, cyh = cyl + (float)(SMH_LBL_TH - 1u);
			const float big = fmaxf(fmaxf(fabsf(c.mx), fabsf(c.my)), fmaxf(cxh, cyh));
			const float rad = c.rad + 1e-5f * big;
			const float ddx = fmaxf(fmaxf(cxl - c.mx, c.mx - cxh), 0.0f), ddy = fmaxf(fmaxf(cyl - c.my, c.my - cyh), 0.0f);
			keep = !(ddx * ddx + ddy * ddy > rad * rad);
		}
	}
	const unsigned long long bal = __ballot(keep);
	if (lane == 0u) s_wave_n[wave] = (uint32_t)__popcll(bal);
	__syncthreads();
	uint32_t base = 0, n_list = 0;
	for (uint32_t w = 0; w < SMH_LBL_WAVES; ++w) {
		if (w < wave) base += s_wave_n[w];
		n_list += s_wave_n[w];
	}
	if (n_list == 0u) return;                                    // (uniform) almost every tile: nothing of the image is touched
	if (keep) s_slot[base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = tid;
	if (tid < SMH_FONT_GLYPHS * SMH_FONT_ROWS) s_font[tid] = ((const uint8_t *)c_font)[tid];
	__syncthreads();
	if (tid < n_list) {
		const smhv_label *sl = &lab->label[s_slot[tid]];
		LblItem *it = &s_item[tid];
		it->mx = sl->mid[0]; it->my = sl->mid[1]; it->ex = sl->dir[0]; it->ey = sl->dir[1];
		it->color = ((const uint32_t *)sl)[16] | 0xFF000000u;
		it->n_runs = min(sl->n_runs, SMH_LBL_RUNS);
	}
	for (uint32_t k = tid; k < n_list * SMH_LBL_RUNS; k += 64u * SMH_LBL_WAVES) {
		const uint32_t i = k / SMH_LBL_RUNS, rr = k - i * SMH_LBL_RUNS;
		const uint32_t *w = (const uint32_t *)&lab->label[s_slot[i]].run[rr];
		const uint32_t w0 = w[0];
		LblItem *it = &s_item[i];
		it->ox[rr] = (float)(int32_t)(int16_t)(w0 & 0xFFFFu) * 0.5f;
		it->oy[rr] = (float)(int32_t)(int16_t)(w0 >> 16) * 0.5f;
		it->wd[rr] = (float)(6u * min(w[1] & 255u, 16u));
		for (uint32_t q = 0; q < 4u; ++q) {
			const uint32_t tw = w[2u + q];
			uint32_t gw = 0u;
			for (uint32_t b = 0; b < 4u; ++b) {
				const int g = smh_font_index((tw >> (8u * b)) & 255u);
				gw |= (uint32_t)(g < 0 ? 24 : g) << (8u * b);          // (the plan writes no other byte; a blank keeps the read in the table)
			}
			((uint32_t *)it->glyph[rr])[q] = gw;
		}
	}
	__syncthreads();

	// ---- the pixels: the list from its end, the first hit is the label painted last ----
	const uint32_t X = tile_x + lane;
	if (X >= r.out_w) return;
	const float fS = (float)r.scale;
	const float cx = (float)X + 0.5f;
	uint32_t *img = (uint32_t *)(r.img + (size_t)f * r.img_stride);
	for (uint32_t j = 0; j < SMH_LBL_TH / SMH_LBL_WAVES; ++j) {
		const uint32_t Y = tile_y + j * SMH_LBL_WAVES + wave;
		if (Y >= r.out_h) break;                                 // (wave-uniform)
		const float cy = (float)Y + 0.5f;
		bool done = false;
		uint32_t color = 0u;
		for (uint32_t li = n_list; li-- > 0u;) {
			const LblItem *it = &s_item[li];
			const float ax = cx - it->mx, ay = cy - it->my;
			const float u = (ax * it->ex + ay * it->ey) / fS;
			const float v = (ay * it->ex - ax * it->ey) / fS;
			bool hit = false;
			const uint32_t nr = it->n_runs;
			for (uint32_t rr = 0; rr < nr; ++rr) {
				const float fu = floorf(u - it->ox[rr]), fv = floorf(v - it->oy[rr]);
				if (0.0f <= fu && fu < it->wd[rr] && 0.0f <= fv && fv < 9.0f) {
					const uint32_t iu = (uint32_t)fu, iv = (uint32_t)fv;
					const uint32_t ch = iu / 6u, col = iu - ch * 6u;
					if (col < 5u && iv >= 1u && iv <= 7u) {
						const uint32_t bits = s_font[(uint32_t)it->glyph[rr][ch] * SMH_FONT_ROWS + (iv - 1u)];
						hit = hit || ((bits >> (4u - col)) & 1u) != 0u;
					}
				}
			}
			if (!done && hit) { done = true; color = it->color; }
		}
		if (done) img[(size_t)Y * r.out_w + X] = color;
	}
}

// at most 65,535 frames per launch of the draw (the grid's third dimension); the plan goes with it chunk by chunk
hipError_t launch_labels(const LabelRun &run, uint32_t n, hipStream_t s) {
	const uint32_t tiles_x = (run.out_w + SMH_LBL_TW - 1u) / SMH_LBL_TW, tiles_y = (run.out_h + SMH_LBL_TH - 1u) / SMH_LBL_TH;
	for (uint32_t done = 0; done < n;) {
		const uint32_t k = n - done < 65535u ? n - done : 65535u;
		LabelRun r = run;
		r.aux += done;
		if (!r.per_call) r.res += done;
		r.out += done;
		r.cull += (size_t)done * SMH_LBL_SLOTS;
		r.img += (size_t)done * r.img_stride;
		hipLaunchKernelGGL(k_label_plan, dim3(k), dim3(128), 0, s, r);
		hipLaunchKernelGGL(k_label_draw, dim3(tiles_x, tiles_y, k), dim3(64u * SMH_LBL_WAVES), 0, s, r);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return e;
		done += k;
	}
	return hipSuccess;
}

}  // namespace smh
