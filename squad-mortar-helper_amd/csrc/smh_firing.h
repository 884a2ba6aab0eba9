// smh_firing.h -- firing solutions of the marker lines: range from the heightmap and the minimap rectangle, altitude difference,
// mils and bearings (src/ui/markers.rs:23-200, src/squadex/milliradians.rs, heightmap-ripper/src/lib.rs:22-25; the semantics are
// spelt out in include/smh_vision_hip.h).  One lane per line.  Device code shared by the record tail (smh_record.inc: the
// batch-granular searches' fused tails, the service's frame_record_tail_wave, k_finalize_firing / k_scales_finalize_firing) and by
// k_firing_lines (smhv_firing_solutions); the same rule restated per axis for a dense pass is k_reach's (smh_reach.hip: reach_axis,
// reach_eval, reach_class below).  Built with -ffp-contract=off: every f32 / f64 operation below is the reference's, in
// its order, unfused.
#pragma once
#include "smh_device.h"

namespace smh {

// VELOCITY.powi(2) and VELOCITY.powi(4) as the Rust build folds them (LLVM evaluates powi of a constant with the host's pow):
// pow(109.890938, 2) and pow(109.890938, 4), not V * V * V * V
#define SMH_MORTAR_V2 0x1.79602562a02dfp+13
#define SMH_MORTAR_V4 0x1.1626291c459a8p+27
#define SMH_MORTAR_G 9.8

// squadex::milliradians::calc (f64): NaN when out of range
__device__ __forceinline__ double mortar_mils(double meters, double alt_delta) {
	const double p1 = sqrt(SMH_MORTAR_V4 - SMH_MORTAR_G * (SMH_MORTAR_G * (meters * meters) + 2.0 * alt_delta * SMH_MORTAR_V2));
	const double a1 = atan((SMH_MORTAR_V2 + p1) / (SMH_MORTAR_G * meters));
	return a1 * (180.0 / 3.14159265358979323846264338327950288) / (360.0 / 6400.0);   // f64::to_degrees, then the mil
}

// Rust `f64.round() as i32`: half away from zero, saturating, NaN -> 0
__device__ __forceinline__ int32_t round_i32(double v) {
	const double r = round(v);
	if (!(r == r)) return 0;
	if (r >= 2147483647.0) return 2147483647;
	if (r <= -2147483648.0) return (-2147483647 - 1);
	return (int32_t)r;
}

// The heightmap's rectangle on the map (src/ui/markers.rs:37-58 == src/ui/heightmaps.rs:802-815): the minimap rectangle mm =
// {left, right, top, bottom} through the viewport (scale sw, sh; top left tx, ty), its top left moved by bounds[0] when "fit to
// minimap" is off (SMHV_FIRING_BOUNDS_OFFSET) -> {left, top, right, bottom} in f32.  The overlay (k_hm_overlay) passes sw = sh = 1,
// tx = ty = 0: (float)v * 1.0f + 0.0f is (float)v.
struct HmRect { float l, t, r, b; };
__device__ __forceinline__ HmRect hm_rect(const uint32_t mm[4], uint32_t flags, float b0x, float b0y, uint32_t hm_w, uint32_t hm_h, float sw, float sh,
                                          float tx, float ty) {
	float off0 = 0.0f, off1 = 0.0f;
	if (flags & SMHV_FIRING_BOUNDS_OFFSET) {
		off0 = b0x * ((float)(mm[1] - mm[0]) / ((float)hm_w + b0x)) * sw;
		off1 = b0y * ((float)(mm[3] - mm[2]) / ((float)hm_h + b0y)) * sh;
	}
	HmRect q;
	q.l = ((float)mm[0] * sw + tx) + off0; q.t = ((float)mm[2] * sh + ty) + off1;
	q.r = (float)mm[1] * sw + tx; q.b = (float)mm[3] * sh + ty;
	return q;
}

// One line.  has_mm / mm: the frame's minimap rectangle {left, right, top, bottom}; met: the record's meters (valid iff has_mpx).
// Both heightmap texels of the lane are loaded together, with no dependent chain between them.
__device__ __forceinline__ smhv_firing firing_line(const FiringRun &r, bool has_mm, const uint32_t mm[4], smhv_line ln, bool has_mpx, double met) {
	smhv_firing o;
	// MapViewport::translate_xy
	const float p0x = ln.x0 * r.sw + r.tx, p0y = ln.y0 * r.sh + r.ty;
	const float p1x = ln.x1 * r.sw + r.tx, p1y = ln.y1 * r.sh + r.ty;
	bool hm_ok = false;
	double hm_m = 0.0, alt = 0.0;
	if (has_mm && r.hm) {
		const HmRect q = hm_rect(mm, r.flags, r.b0x, r.b0y, r.hm_w, r.hm_h, r.sw, r.sh, r.tx, r.ty);
		const float rl = q.l, rt = q.t, rr = q.r, rb = q.b;
		const double rw = (double)(rr - rl), rh = (double)(rb - rt);
		const double x0 = (((double)p0x - (double)rl) / rw) * (double)r.hm_w, y0 = (((double)p0y - (double)rt) / rh) * (double)r.hm_h;
		const double x1 = (((double)p1x - (double)rl) / rw) * (double)r.hm_w, y1 = (((double)p1y - (double)rt) / rh) * (double)r.hm_h;
		const double dx = x0 - x1, dy = y0 - y1;
		hm_m = sqrt(dx * dx + dy * dy);
		const int32_t ix0 = round_i32(x0), iy0 = round_i32(y0), ix1 = round_i32(x1), iy1 = round_i32(y1);
		const int32_t W = (int32_t)r.hm_w, H = (int32_t)r.hm_h;
		hm_ok = ix0 >= 0 && iy0 >= 0 && ix1 >= 0 && iy1 >= 0 && ix0 < W && iy0 < H && ix1 < W && iy1 < H;
		// both texels in one round trip (texel 0 stands in for an end point outside the map)
		const size_t i0 = hm_ok ? (size_t)iy0 * r.hm_w + (size_t)ix0 : 0u, i1 = hm_ok ? (size_t)iy1 * r.hm_w + (size_t)ix1 : 0u;
		const uint16_t v0 = r.hm[i0], v1 = r.hm[i1];
		const double h0 = ((double)v0 / 65535.0) * r.zscale, h1 = ((double)v1 / 65535.0) * r.zscale;
		alt = h1 - h0;
	}
	uint32_t source = SMHV_FIRING_NONE;
	double meters = 0.0;
	if (hm_ok) { source = SMHV_FIRING_HEIGHTMAP; meters = hm_m; }
	else if (has_mpx) { source = SMHV_FIRING_SCALES; meters = met; alt = 0.0; }
	else alt = 0.0;
	o.meters = meters;
	o.alt_delta = alt;
	if (source != SMHV_FIRING_NONE) {
		o.mils[0] = mortar_mils(meters, alt);
		o.mils[1] = mortar_mils(meters, -alt);
	} else {
		o.mils[0] = 0.0; o.mils[1] = 0.0;
	}
	// bearings (markers.rs:98-110): f32::to_degrees, then whole degrees half away from zero, mod 360
	const float angle = atan2f(p0y - p1y, p0x - p1x);
	float d = angle * 57.2957795130823208767981548141051703f;
	if (d > 0.0f) {
		d -= 90.0f;
		if (d < 0.0f) d += 360.0f;
	} else {
		d += 270.0f;
	}
	const float fwd = fmodf(roundf(d), 360.0f);
	o.bearing[0] = fwd;
	o.bearing[1] = fmodf(roundf(fwd + 180.0f), 360.0f);
	o.source = source;
	o.reserved = 0u;
	return o;
}

// ---- the reach map (k_reach, smh_reach.hip): firing_line()'s rule for the line (origin, the target of a window pixel), direction 0,
// restated per axis -- the heightmap coordinate of a pixel depends on its column or its row alone, and so do the scales branch's
// differences.  The operations are firing_line()'s, one for one; what is not needed (bearings, the reverse direction, atan) is left out.
// One axis of a pixel at centre c (cx or cy): o = the origin's coordinate, s / t = the viewport's scale and top left on this axis,
// r0 / rlen = the heightmap rectangle's near edge and its length as firing_line() takes them, n = the heightmap's texels on this axis.
struct ReachAxis {
	double dh;        // heightmap branch: coordinate of the origin minus coordinate of the target (firing_line's dx / dy)
	double ds;        // scales branch: (double)o - (double)target
	int32_t ix;       // the target's rounded heightmap coordinate; -1 unless it AND the origin's lie inside [0, n) and a heightmap applies
	uint32_t fin;     // the target's coordinate is finite
};
__device__ __forceinline__ ReachAxis reach_axis(float c, float o, float s, float t, bool use_hm, float r0, double rlen, uint32_t n) {
	ReachAxis a;
	const float tg = (c - t) / s;                                // MapViewport::inverse_xy
	const float p0 = o * s + t, p1 = tg * s + t;                   // MapViewport::translate_xy
	a.fin = isfinite(tg) ? 1u : 0u;
	a.ds = (double)o - (double)tg;
	a.dh = 0.0;
	a.ix = -1;
	if (use_hm) {
		const double c0 = (((double)p0 - (double)r0) / rlen) * (double)n, c1 = (((double)p1 - (double)r0) / rlen) * (double)n;
		a.dh = c0 - c1;
		const int32_t i0 = round_i32(c0), i1 = round_i32(c1), N = (int32_t)n;
		if (i0 >= 0 && i0 < N && i1 >= 0 && i1 < N) a.ix = i1;
	}
	return a;
}
// the origin's own rounded heightmap coordinate on one axis (-1: outside)
__device__ __forceinline__ int32_t reach_origin_texel(float o, float s, float t, float r0, double rlen, uint32_t n) {
	const float p0 = o * s + t;
	const int32_t i0 = round_i32((((double)p0 - (double)r0) / rlen) * (double)n);
	return i0 >= 0 && i0 < (int32_t)n ? i0 : -1;
}
// What decides a pixel's class but for the altitude: source (NONE also where the class would be 0 for another reason), meters and,
// with rings, floor(meters / ring_m).
struct ReachEval { double m, b; uint32_t src; };
__device__ __forceinline__ ReachEval reach_eval(const ReachAxis &c, const ReachAxis &r, bool has_mpx, double mpx, bool rings, double ring_m) {
	const bool hm = c.ix >= 0 && r.ix >= 0;
	const double dx = hm ? c.dh : c.ds, dy = hm ? r.dh : r.ds;
	const double len = sqrt(dx * dx + dy * dy);
	ReachEval e;
	e.m = hm ? len : len * mpx;
	e.src = hm ? SMHV_FIRING_HEIGHTMAP : has_mpx ? SMHV_FIRING_SCALES : SMHV_FIRING_NONE;
	if (!(c.fin & r.fin) || !(e.m == e.m)) e.src = SMHV_FIRING_NONE;
	e.b = rings ? floor(e.m / ring_m) : 0.0;
	return e;
}
// the class of a pixel with a source: 1 = out of range (mortar_mils() would be NaN), 2 + k = band k (header, "reach map")
__device__ __forceinline__ uint32_t reach_class(double meters, double alt_delta) {
	const double T[7] = SMH_REACH_THRESHOLDS;
	const double disc = SMH_MORTAR_V4 - SMH_MORTAR_G * (SMH_MORTAR_G * (meters * meters) + 2.0 * alt_delta * SMH_MORTAR_V2);
	const double q = (SMH_MORTAR_V2 + sqrt(disc)) / (SMH_MORTAR_G * meters);   // (NaN when out of range: no threshold is met)
	uint32_t k = 0u;
#pragma unroll
	for (int j = 0; j < 7; ++j) k += q >= T[j] ? 1u : 0u;
	return disc >= 0.0 ? SMHV_REACH_BAND0 + k : SMHV_REACH_OUT_OF_RANGE;
}

// the paint of the reach map and of the clearance map: palette entry pal (R, G, B, a as a little-endian word) over pixel px, alpha kept
__device__ __forceinline__ uint32_t reach_blend(uint32_t px, uint32_t pal) {
	const uint32_t a = pal >> 24, na = 255u - a;
	const uint32_t r = ((px & 255u) * na + (pal & 255u) * a + 127u) / 255u;
	const uint32_t g = (((px >> 8) & 255u) * na + ((pal >> 8) & 255u) * a + 127u) / 255u;
	const uint32_t b = (((px >> 16) & 255u) * na + ((pal >> 16) & 255u) * a + 127u) / 255u;
	return (px & 0xFF000000u) | (b << 16) | (g << 8) | r;
}

// ---- terrain clearance (k_clear_lines, k_clear_map: smh_clear.hip): the header's "terrain clearance", one function per step of its
// rule, so the per-line and the dense kernel run the same operations.
// The heightmap coordinate of a translated point on one axis, as firing_line() and reach_axis() compute it.
__device__ __forceinline__ double clear_coord(float p, float r0, double rlen, uint32_t n) { return (((double)p - (double)r0) / rlen) * (double)n; }
// (double)v / 65535.0 * zscale.  The quotient of a 16-bit v is formed without the division's instruction sequence: q0 = v * r with
// r = RN(1 / 65535), rem = v - q0 * 65535 exactly (one fma), q = q0 + rem * r (one more).  That is the IEEE quotient, bit for bit, for
// every one of the 65,536 inputs (tests/test_clearance_host.py runs them all through the host's fma) at 3 instructions in place of 11;
// the texel's height is what every sample of the march computes first.
#define SMH_RCP_65535 0x1.000100010001p-16
__device__ __forceinline__ double clear_height(uint16_t v, double zscale) {
	const double n = (double)v, q0 = n * SMH_RCP_65535;
	return fma(fma(-q0, 65535.0, n), SMH_RCP_65535, q0) * zscale;
}
// sample k's rounded, clamped texel coordinate on one axis: c0, c1 = the end coordinates, t = (double)k / (double)S
__device__ __forceinline__ uint32_t clear_texel(double c0, double c1, double t, uint32_t n) {
	const int32_t i = round_i32(c0 + (c1 - c0) * t);
	return (uint32_t)min(max(i, 0), (int32_t)n - 1);
}
// What a line's samples are held against: d, alt, disc, q and 1 + q * q (the rule's steps 1 and 2)
struct ClearArc { double d, alt, disc, q, qq1; };
__device__ __forceinline__ ClearArc clear_arc(double d, double alt) {
	ClearArc c;
	c.d = d; c.alt = alt;
	c.disc = SMH_MORTAR_V4 - SMH_MORTAR_G * (SMH_MORTAR_G * (d * d) + 2.0 * alt * SMH_MORTAR_V2);
	c.q = (SMH_MORTAR_V2 + sqrt(c.disc)) / (SMH_MORTAR_G * d);
	c.qq1 = 1.0 + c.q * c.q;
	return c;
}
// One sample (step 3): z = the terrain over the origin there -> the margin m; *los = the sample blocks the sight line
__device__ __forceinline__ double clear_sample(const ClearArc &c, double t, double z, bool *los) {
	const double x = c.d * t;
	const double a = x * c.q - ((SMH_MORTAR_G * (x * x)) * c.qq1) / (2.0 * SMH_MORTAR_V2);
	*los = c.alt * t < z;
	return a - z;
}

// The frame's firing slab from its finished record: lane l (< 64) takes line l.  Called by one wave after a wave barrier behind
// lane 0's header writes (the record is read back: n_lines, m/px, the minimap rectangle and the line's own fields).
__device__ __forceinline__ void firing_frame_tail(const Buffers *bp, uint32_t f, uint32_t lane) {
	const FiringRun *rp = bp->firing;
	const smhv_frame_result *res = &bp->results[f];
	const uint32_t n = res->n_lines, has_mpx = res->has_mpx, has_mm = res->has_minimap;
	const uint32_t mm[4] = {res->minimap[0], res->minimap[1], res->minimap[2], res->minimap[3]};
	const FiringRun r = *rp;
	smhv_firing_result *out = &r.out[f];
	if (lane < SMHV_MAX_LINES) {
		smhv_firing o{};
		if (lane < n) o = firing_line(r, has_mm != 0u, mm, res->lines[lane], has_mpx != 0u, res->meters[lane]);
		out->line[lane] = o;
	}
	if (lane == 0) { out->n_lines = n; out->reserved = 0u; }
}

}  // namespace smh
