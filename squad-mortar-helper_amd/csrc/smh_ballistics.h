// smh_ballistics.h -- the rule of "ballistics" (include/smh_vision_hip.h): a caller-supplied weapon in the rule's terms, the two roots
// of its firing solution from (meters, alt), and per root the elevation, the time of flight, the apex, the tangent of the angle of
// fall, the dispersion's half widths, the status bits and the elevation band; below them the per-arc steps of "ballistic clearance".  One text for the kernels (smh_ballistics.hip, smh_balclear.hip), the host
// entry points (smh_ballistics.inc) and a stand-alone host check (tests/ballistics_rule_check.cpp compiles this header with the host
// compiler), hence SMH_HD.  Built with -ffp-contract=off: every f64 operation below is the header's, in its order, unfused.  Below the
// rule, for the HIP build alone: the launch interface of smh_ballistics.hip (the run structs live here and not in smh_kernels.h, which
// every other kernel file includes).
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

#define SMH_BAL_DEG_PER_RAD (180.0 / 3.14159265358979323846264338327950288)   // f64::to_degrees' factor, as mortar_mils() writes it
#define SMH_BAL_RAD_PER_DEG 0x1.1df46a2529d39p-6                              // pi / 180.0
#define SMH_BAL_QUARTER_TURN 0x1.921fb54442d18p+0                             // pi / 2.0

// ---- the weapon in the rule's terms: host only (pow and tan are the C library's; nothing here runs on a device)
static inline bool weapon_ok(const smhv_weapon *w) {
	if (!w || w->size != sizeof(smhv_weapon)) return false;
	if (w->arc > SMHV_ARC_LOW || w->unit > SMHV_ANGLE_DEGREES) return false;
	if (!(isfinite(w->velocity) && w->velocity > 0.0) || !(isfinite(w->gravity) && w->gravity > 0.0)) return false;
	if (!isfinite(w->elev_min) || !isfinite(w->elev_max) || w->elev_min > w->elev_max) return false;
	if (!(isfinite(w->range_min) && w->range_min >= 0.0) || !(isfinite(w->dispersion) && w->dispersion >= 0.0)) return false;
	return true;
}
static inline double weapon_tanlim(double e, double unit_deg) {
	const double r = (e * unit_deg) * SMH_BAL_RAD_PER_DEG;
	if (r >= SMH_BAL_QUARTER_TURN) return (double)INFINITY;
	if (r <= -SMH_BAL_QUARTER_TURN) return -(double)INFINITY;
	return tan(r);
}
static inline void weapon_rule(const smhv_weapon *w, smhv_weapon_rule *o) {
	volatile double two = 2.0, four = 4.0;                         // (the library's pow, not a product the compiler makes of it)
	memset(o, 0, sizeof *o);
	o->v = w->velocity; o->g = w->gravity;
	o->v2 = pow(w->velocity, two); o->v4 = pow(w->velocity, four);
	o->unit_deg = w->unit == SMHV_ANGLE_MILS6400 ? 360.0 / 6400.0 : w->unit == SMHV_ANGLE_MILS6000 ? 360.0 / 6000.0 : 1.0;
	o->t_min = weapon_tanlim(w->elev_min, o->unit_deg);
	o->t_max = weapon_tanlim(w->elev_max, o->unit_deg);
	for (int j = 0; j < 7; ++j) o->band[j] = weapon_tanlim(w->elev_min + ((w->elev_max - w->elev_min) * (double)(j + 1)) / 8.0, o->unit_deg);
	o->t_disp = tan(w->dispersion);
	o->range_min = w->range_min;
	o->arc = w->arc; o->unit = w->unit;
}

// ---- a solution, piece by piece (the map kernel takes the pieces it needs; bal_solve takes them all)
SMH_HD double bal_disc(const smhv_weapon_rule &w, double m, double alt) { return w.v4 - w.g * (w.g * (m * m) + 2.0 * alt * w.v2); }
// the root of one arc: s = sqrt(disc), gm = g * m
SMH_HD double bal_root(const smhv_weapon_rule &w, double s, double gm, uint32_t arc) { return arc == SMHV_ARC_HIGH ? (w.v2 + s) / gm : (w.v2 - s) / gm; }
SMH_HD uint32_t bal_status(const smhv_weapon_rule &w, double disc, double m, double T) {
	uint32_t st = m < w.range_min ? SMHV_BAL_BELOW_MIN_RANGE : 0u;
	if (!(disc >= 0.0)) return st | SMHV_BAL_OUT_OF_RANGE;
	if (!(T >= w.t_min)) st |= SMHV_BAL_ELEV_LOW;
	if (!(w.t_max >= T)) st |= SMHV_BAL_ELEV_HIGH;
	return st;
}
SMH_HD uint32_t bal_band(const smhv_weapon_rule &w, double T) {
	return (T >= w.band[0] ? 1u : 0u) + (T >= w.band[1] ? 1u : 0u) + (T >= w.band[2] ? 1u : 0u) + (T >= w.band[3] ? 1u : 0u) + (T >= w.band[4] ? 1u : 0u) +
	       (T >= w.band[5] ? 1u : 0u) + (T >= w.band[6] ? 1u : 0u);
}
SMH_HD double bal_tof(const smhv_weapon_rule &w, double m, double T) { return (m * sqrt(1.0 + T * T)) / w.v; }
// the map's class byte without the isochrone bit, of a pixel that has a source
SMH_HD uint32_t bal_class(uint32_t st, uint32_t band) {
	return (st & SMHV_BAL_OUT_OF_RANGE) ? SMHV_BMAP_OUT_OF_RANGE : (st & SMHV_BAL_BELOW_MIN_RANGE) ? SMHV_BMAP_BELOW_MIN_RANGE :
	       (st & SMHV_BAL_ELEV_LOW) ? SMHV_BMAP_ELEV_LOW : (st & SMHV_BAL_ELEV_HIGH) ? SMHV_BMAP_ELEV_HIGH : SMHV_BMAP_BAND0 + band;
}
SMH_HD smhv_ballistic_arc bal_arc(const smhv_weapon_rule &w, double m, double gm, double disc, double T) {
	smhv_ballistic_arc a;
	const double tt = T * T;
	a.elevation = (atan(T) * SMH_BAL_DEG_PER_RAD) / w.unit_deg;
	a.tof = (m * sqrt(1.0 + tt)) / w.v;
	a.apex = T <= 0.0 ? 0.0 : (w.v2 * tt) / ((1.0 + tt) * (2.0 * w.g));
	a.fall = (gm * (1.0 + tt)) / w.v2 - T;
	a.along = fabs(((m * (1.0 - (gm * T) / w.v2)) * (1.0 + tt)) / a.fall) * w.t_disp;
	a.status = bal_status(w, disc, m, T);
	a.band = bal_band(w, T);
	return a;
}
SMH_HD smhv_ballistic_solution bal_solve(const smhv_weapon_rule &w, double m, double alt, uint32_t source) {
	smhv_ballistic_solution o;
	const double disc = bal_disc(w, m, alt), s = sqrt(disc), gm = w.g * m;
	o.meters = m; o.alt_delta = alt;
	o.cross = m * w.t_disp;
	o.source = source; o.reserved = 0u;
	o.arc[SMHV_ARC_HIGH] = bal_arc(w, m, gm, disc, bal_root(w, s, gm, SMHV_ARC_HIGH));
	o.arc[SMHV_ARC_LOW] = bal_arc(w, m, gm, disc, bal_root(w, s, gm, SMHV_ARC_LOW));
	return o;
}

// ---- "ballistic clearance" (smh_balclear.hip, tests/ballistic_clearance_rule_check.cpp): both arcs of the weapon held against the
// terrain, one function per step of the header's rule so that the per-line kernel, the dense kernel and the host program run the same
// operations.  What the two arcs share (t, the texel, z, x, w.g * (x * x)) is the caller's; what follows is per arc.
// One arc of a line: its root, 1 + T * T and its status bits (s = sqrt(disc), gm = w.g * d)
struct BalClearArc { double T, qq1; uint32_t bal; };
SMH_HD BalClearArc bal_clear_arc(const smhv_weapon_rule &w, double disc, double s, double gm, double d, uint32_t arc) {
	BalClearArc a;
	a.T = bal_root(w, s, gm, arc);
	a.qq1 = 1.0 + a.T * a.T;
	a.bal = bal_status(w, disc, d, a.T);
	return a;
}
// One sample against one arc: x = d * t, gxx = w.g * (x * x), den = 2.0 * w.v2, z = the terrain over the origin -> the margin m
SMH_HD double bal_clear_sample(double x, double gxx, double T, double qq1, double den, double z) {
	const double a = x * T - (gxx * qq1) / den;
	return a - z;
}
// the sample blocks the sight line
SMH_HD bool bal_clear_los(double alt, double t, double z) { return alt * t < z; }
// an arc's status in the line record, its class in the map's byte (blocked: some sample blocked it)
SMH_HD uint32_t bal_clear_status(bool oor, bool none, bool blocked) {
	return oor ? SMHV_CLEAR_OUT_OF_RANGE : (!none && blocked) ? SMHV_CLEAR_BLOCKED : SMHV_CLEAR_CLEAR;
}
SMH_HD uint32_t bal_clear_class(bool oor, bool none, uint32_t bal, bool blocked) {
	return oor ? SMHV_BCLR_OUT_OF_RANGE : bal ? SMHV_BCLR_UNUSABLE : (!none && blocked) ? SMHV_BCLR_BLOCKED : SMHV_BCLR_CLEAR;
}
// the arc to fire as 1 + a, or 0: the weapon's own if it is CLEAR and usable, else the other one under the same condition
SMH_HD uint32_t bal_clear_choice(uint32_t own, const uint32_t status[2], const uint32_t bal[2]) {
	const uint32_t other = 1u - own;
	if (status[own] == SMHV_CLEAR_CLEAR && bal[own] == 0u) return 1u + own;
	if (status[other] == SMHV_CLEAR_CLEAR && bal[other] == 0u) return 1u + other;
	return 0u;
}
// min_margin as a record reports it: 0 when nothing replaced the starting +inf (no arc, no samples, S == 1, every m a NaN)
SMH_HD double bal_clear_margin(double best) { return best == (double)INFINITY ? 0.0 : best; }

}  // namespace smh

// ---- the launch interface of smh_ballistics.hip
#if defined(__HIPCC__)
#include "smh_kernels.h"
namespace smh {
// smhv_batch_ballistics / smhv_ballistic_lines (k_ballistic_lines): launch arguments, taken by value at the launch
struct BalLinesRun {
	FiringRun fr;                        // the heightmap and the viewport, as the firing solutions take them (`out` is not used)
	smhv_weapon_rule w;
	const smhv_frame_result *res;        // batch, per frame: n_lines, the lines, their meters, m/px, the minimap rectangle
	const smhv_line *lines;              // per call: the explicit lines
	smhv_ballistic_result *out;          // batch: the ballistics slab, at the first frame of the call
	smhv_ballistic *out_lines;           // per call: one record per line
	double mpx;                          // per call: the frame's meters per pixel (valid iff has_mpx)
	uint32_t n_lines;                    // per call: of `lines`
	uint32_t mm[4];                      // per call: the minimap rectangle (valid iff has_mm)
	uint32_t per_call, has_mm, has_mpx;
};
// smhv_batch_ballistic_map / smhv_ballistic_map (k_ballistic_map, k_ballistic_finish): the ballistic map of n frames, in k_reach's tiles
struct BalMapRun {
	FiringRun fr;
	smhv_weapon_rule w;
	const FrameAux *aux;                 // batch, per frame: open
	const smhv_frame_result *res;        // batch, per frame: m/px, the minimap rectangle, the lines (the origin)
	smhv_ballistic_map_result *out;      // the slab, at the first frame of the call; cleared ahead of the launch
	uint8_t *img;                        // PAINT: the render slab, at the first frame of the call
	uint8_t *cls;                        // the planes (null: not asked for): out_w * out_h elements per frame
	float *tof;
	uint64_t img_stride, plane_stride;   // out_w * out_h * 4 bytes, out_w * out_h elements
	double mpx;                          // per call: the frame's meters per pixel (valid iff has_mpx)
	double iso_s;
	float origin[2];                     // SMHV_REACH_ORIGIN_POINT
	uint32_t mm[4];                      // per call: the minimap rectangle (valid iff has_mm)
	uint32_t out_w, out_h;
	uint32_t origin_mode, line;
	uint32_t per_call, has_mpx, has_mm;  // 1: mpx / has_mpx, mm / has_mm are the call's and aux, res are not read
	uint32_t pal[13];                    // classes 1 .. 12, iso: R, G, B, a as a little-endian word
};
// k_ballistic_lines over n frames x SMHV_MAX_LINES lines x 2 directions (per call: n = 1, r.n_lines lines)
hipError_t launch_ballistic_lines(const BalLinesRun &r, uint32_t n, hipStream_t s);
// k_ballistic_map<paint, planes> over n frames (at most 65,535), then k_ballistic_finish over their summaries; the planes asked for are
// the non-null pointers of r
hipError_t launch_ballistic_map(const BalMapRun &r, uint32_t n, bool paint, hipStream_t s);

// ---- the launch interface of smh_balclear.hip
// smhv_batch_ballistic_clearance / smhv_ballistic_clearance_lines (k_bclear_lines): ClearLinesRun's fields and the weapon
struct BalClearLinesRun {
	FiringRun fr;                        // the heightmap and the viewport, as the firing solutions take them (`out` is not used)
	smhv_weapon_rule w;
	const smhv_frame_result *res;        // batch, per frame: n_lines, the lines, the minimap rectangle
	const smhv_line *lines;              // per call: the explicit lines
	smhv_ballistic_clearance_result *out;   // batch: the slab, at the first frame of the call
	smhv_ballistic_clearance *out_lines; // per call: one record per line
	double margin_m;
	uint32_t samples;                    // S
	uint32_t n_lines;                    // per call: of `lines`
	uint32_t mm[4];                      // per call: the minimap rectangle (valid iff has_mm)
	uint32_t per_call, has_mm;
};
// smhv_batch_ballistic_clearance_map / smhv_ballistic_clearance_map (k_bclear_map): ClearMapRun's fields, the weapon and the planes
#define SMH_BCLR_ROWS 2u                 // rows per lane: a tile of SMH_REACH_TW x SMH_REACH_TH is 8 waves
#define SMH_BCLR_THREADS (64u * (SMH_REACH_TH / SMH_BCLR_ROWS))
struct BalClearMapRun {
	FiringRun fr;
	smhv_weapon_rule w;
	const FrameAux *aux;                 // batch, per frame: open
	const smhv_frame_result *res;        // batch, per frame: the minimap rectangle, the lines (the origin)
	smhv_ballistic_clearance_map_result *out;   // the slab, at the first frame of the call; cleared ahead of the launch
	uint8_t *img;                        // PAINT: the render slab, at the first frame of the call
	uint8_t *bytes;                      // the planes (null: not asked for): out_w * out_h elements per frame
	float *margin;
	uint64_t img_stride, plane_stride;   // out_w * out_h * 4 bytes, out_w * out_h elements
	double margin_m;
	float origin[2];                     // SMHV_REACH_ORIGIN_POINT
	uint32_t mm[4];                      // per call: the minimap rectangle (valid iff has_mm)
	uint32_t out_w, out_h;
	uint32_t samples;                    // S
	uint32_t origin_mode, line;
	uint32_t per_call, has_mm;           // 1: mm / has_mm are the call's and aux, res are not read
	uint32_t pal[6];                     // own classes 1 .. 4, switch_arc, los: R, G, B, a as a little-endian word
};
// k_bclear_lines over n frames x SMHV_MAX_LINES lines x 2 directions (per call: n = 1, r.n_lines lines)
hipError_t launch_bclear_lines(const BalClearLinesRun &r, uint32_t n, hipStream_t s);
// k_bclear_map<paint, planes> over n frames (at most 65,535); the planes asked for are the non-null pointers of r
hipError_t launch_bclear_map(const BalClearMapRun &r, uint32_t n, bool paint, hipStream_t s);
}  // namespace smh
#endif
