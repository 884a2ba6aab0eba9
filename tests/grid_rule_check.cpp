// grid_rule_check.cpp -- csrc/smh_grid.h as a stand-alone host program (tests/test_grid_host.py builds it with the host compiler,
// with -fsanitize=address,undefined where that links, and holds its output against tests/grid_ref.py index for index, digit for
// digit, string for string).
//   grid_rule_check in.bin out.bin
// in.bin:  u32 jobs, then per job a JobIn and `n` PointIn.
// out.bin: per job a JobOut, then per point a PointOut.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "smh_grid.h"

using namespace smh;

struct JobIn {
	double mpx, origin[2], cell_m, min_px, label_min_px;
	float r0[2], r1[2], s[2];
	uint32_t n_tex[2];
	uint32_t scales;                     // 1: the scales branch
	uint32_t L, label_weight, n;
};
struct PointIn {
	float x, y;
	int32_t X, Y;                        // the pixel whose centre (x, y) is, or INT32_MIN: a free point
};
struct JobOut { int32_t Ld; uint32_t labels; };
struct PointOut {
	smhv_grid_ref ref;
	int32_t idx[2];
	uint32_t flags;                      // in_x | has_x << 1 | in_y << 2 | has_y << 3
	int32_t first[2];                    // grid_first of the pixel's column and row (0: not a pixel, or no index)
	uint32_t cross[2];                   // grid_cross of (X, X + 1) and (Y, Y + 1), 4 where an entry has no index
	uint32_t pad;
};
static_assert(sizeof(JobIn) == 96 && sizeof(PointIn) == 16 && sizeof(JobOut) == 8 && sizeof(PointOut) == 80, "the layouts the test packs");

static bool read_all(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
	if (argc != 3) { fprintf(stderr, "usage: grid_rule_check in.bin out.bin\n"); return 2; }
	FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
	if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
	uint32_t jobs = 0;
	if (!read_all(in, &jobs, 4)) return 2;
	size_t points = 0;
	for (uint32_t j = 0; j < jobs; ++j) {
		JobIn ji;
		if (!read_all(in, &ji, sizeof ji)) { fprintf(stderr, "job %u: short input\n", j); return 2; }
		std::vector<PointIn> pts(ji.n);
		if (ji.n && !read_all(in, pts.data(), sizeof(PointIn) * ji.n)) { fprintf(stderr, "job %u: short points\n", j); return 2; }
		GridAxis a[2];
		for (int k = 0; k < 2; ++k)
			a[k] = ji.scales ? grid_axis_scales(ji.r0[k], ji.r1[k], ji.s[k], ji.mpx, ji.origin[k], ji.cell_m, ji.L)
			                 : grid_axis_heightmap(ji.r0[k], ji.r1[k], ji.n_tex[k], ji.origin[k], ji.cell_m, ji.L);
		JobOut jo;
		jo.Ld = grid_drawn_levels(ji.cell_m, ji.L, a[0].ppm, a[1].ppm, ji.min_px);
		jo.labels = grid_labels_drawn(ji.cell_m, a[0], a[1], jo.Ld, ji.label_weight, ji.label_min_px) ? 1u : 0u;
		fwrite(&jo, sizeof jo, 1, out);
		for (const PointIn &p : pts) {
			PointOut po;
			memset(&po, 0, sizeof po);
			po.ref = grid_ref_of(a[0], a[1], p.x, p.y);
			const float c[2] = {p.x, p.y};
			const int32_t P[2] = {p.X, p.Y};
			for (int k = 0; k < 2; ++k) {
				const GridIdx e = grid_index(a[k], c[k]);
				po.idx[k] = e.idx;
				po.flags |= (e.in | e.has << 1) << (2 * k);
				po.cross[k] = 4u;
				if (P[k] == INT32_MIN || !e.has) continue;
				po.first[k] = grid_first(a[k], P[k], grid_level(e.idx, ji.L, 0u));
				const GridIdx nx = grid_index(a[k], (float)(P[k] + 1) + 0.5f);
				if (nx.has) po.cross[k] = grid_cross(e.idx, nx.idx, ji.L, jo.Ld);
			}
			fwrite(&po, sizeof po, 1, out);
			++points;
		}
	}
	fclose(in);
	if (fclose(out) != 0) return 2;
	printf("ok: %u jobs, %zu points\n", jobs, points);
	return 0;
}
