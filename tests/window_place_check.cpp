// window_place_check.cpp -- a stand-alone CPU program (tests/test_window_reuse_host.py builds and runs it) that holds the window
// placement rule of squad-mortar-helper_amd/csrc/smh_window_place.h against a pixel-wise statement of what it must mean.
//
//   window_place_check 0        the header's predicate: exit 0 when every check passes
//   window_place_check 1 .. 4   a mutant -- the predicate asked about a window one row higher / lower, one word further left / right
//                               than the one that is stored: the checks must FAIL (exit 1)
//
// For every candidate (px, py) of a 256 x 256 corner region and of an 8 px strip along each border of a 1920 x 1080 and a 2560 x 1440
// frame's map ROI, every E in {0, 8, 24}, and every stored placement a fill can have produced that lies close enough to matter (word
// columns within 3 of the candidate's own, first rows from rows + 2 above the candidate's own to 2 below; every other producible word
// column at the candidate's own first row):
//   holds  =>  every pixel column of [px - R, px + R] lies in one of the stored words and every row of [py - R, py + R] is a stored row
//   the region contained  =>  holds (the rule gives no reuse away; not asked of the mutants, which are there to fail the first)
// and the placement of a fresh fill holds its own candidate.
#include <cstdio>
#include <cstdlib>
#include "smh_window_place.h"

static int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

static int g_dx = 0, g_dy = 0;
static bool holds_under_test(int x0w, int y0, int rows, int px, int py) { return smh_window_holds(x0w + g_dx, y0 + g_dy, rows, px, py); }

// the needed region, pixel by pixel: the words its columns fall into and its rows (once per candidate)
struct Needed { int w_lo, w_hi, y_lo, y_hi; };
static Needed needed(int px, int py) {
	Needed n = {1 << 30, -(1 << 30), py - SMH_WIN_R, py - SMH_WIN_R};
	for (int x = px - SMH_WIN_R; x <= px + SMH_WIN_R; ++x) {
		const int w = floor_div(x, 32);
		if (w < n.w_lo) n.w_lo = w;
		if (w > n.w_hi) n.w_hi = w;
	}
	for (int y = py - SMH_WIN_R; y <= py + SMH_WIN_R; ++y) n.y_hi = y;
	return n;
}
// the stored rectangle (SMH_WIN_WORDS words from x0w, `rows` rows from y0) contains it
static bool contains(int x0w, int y0, int rows, const Needed &n) {
	return x0w <= n.w_lo && n.w_hi < x0w + SMH_WIN_WORDS && y0 <= n.y_lo && n.y_hi < y0 + rows;
}

static long long g_checks = 0;
static int fail(const char *what, int rw, int rh, int e, int px, int py, int x0w, int y0) {
	std::printf("FAILED: %s: ROI %d x %d, E = %d, candidate (%d, %d), window at word %d, row %d\n", what, rw, rh, e, px, py, x0w, y0);
	return 1;
}

static int check_candidate(int rw, int rh, int e, int px, int py) {
	const int rows = 2 * SMH_WIN_R + 1 + e;
	const Needed n = needed(px, py);
	int fx, fy;
	smh_window_fresh(px, py, &fx, &fy);
	if (fx != floor_div(px - SMH_WIN_R, 32) || fy != py - SMH_WIN_R) return fail("a fresh window's placement", rw, rh, e, px, py, fx, fy);
	// the placements fills can have produced: fresh windows of the ROI's pixels
	const int xw_lo = floor_div(0 - SMH_WIN_R, 32), xw_hi = floor_div(rw - 1 - SMH_WIN_R, 32), y_lo = -SMH_WIN_R, y_hi = rh - 1 - SMH_WIN_R;
	for (int x0w = xw_lo; x0w <= xw_hi; ++x0w) {
		const bool near_x = x0w >= fx - 3 && x0w <= fx + 3;
		for (int y0 = near_x ? fy - rows - 2 : fy; y0 <= (near_x ? fy + 2 : fy); ++y0) {
			if (y0 < y_lo || y0 > y_hi) continue;
			++g_checks;
			const bool h = holds_under_test(x0w, y0, rows, px, py), c = contains(x0w, y0, rows, n);
			if (h && !c) return fail("holds, but the stored rectangle does not contain the needed region", rw, rh, e, px, py, x0w, y0);
			if (c && !h && !g_dx && !g_dy) return fail("the stored rectangle contains the needed region, but does not hold", rw, rh, e, px, py, x0w, y0);
		}
	}
	if (!holds_under_test(fx, fy, rows, px, py) || !contains(fx, fy, rows, n)) return fail("a fresh window does not hold its own candidate", rw, rh, e, px, py, fx, fy);
	return 0;
}

int main(int argc, char **argv) {
	const int mutant = argc > 1 ? std::atoi(argv[1]) : 0;
	g_dy = mutant == 1 ? -1 : mutant == 2 ? 1 : 0;
	g_dx = mutant == 3 ? -1 : mutant == 4 ? 1 : 0;
	const int rois[2][2] = {{986, 822}, {1314, 1096}};                  // map_bounds of 1920 x 1080 and 2560 x 1440
	const int extra[3] = {0, 8, 24};
	for (const auto &roi : rois) {
		const int rw = roi[0], rh = roi[1];
		for (int e : extra) {
			for (int py = 0; py < rh; ++py) {
				for (int px = 0; px < rw; ++px) {
					const bool corner = px < 256 && py < 256;
					const bool strip = px < 8 || py < 8 || px >= rw - 8 || py >= rh - 8;
					if (!corner && !strip) { if (py >= 8 && py < rh - 8 && px >= 8 && px < rw - 8) px = rw - 9; continue; }
					if (check_candidate(rw, rh, e, px, py)) return 1;
				}
			}
		}
	}
	std::printf("ok: %lld placements checked\n", g_checks);
	return 0;
}
