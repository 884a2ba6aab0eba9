// ballistic_clearance_rule_check.cpp -- the "ballistic clearance" steps of csrc/smh_ballistics.h as a stand-alone host program
// (tests/test_ballistic_clearance_host.py builds it with the host compiler, with -fsanitize=address,undefined where that links, and holds
// its output against tests/ballistic_clearance_ref.py bit for bit).  One job is one direction of one line: the weapon, d, alt, S, the
// margin and the terrain z over the origin at every interior sample, marched sequentially -- the order the kernels' reductions have to
// reproduce.
//   ballistic_clearance_rule_check in.bin out.bin
// in.bin:  u32 jobs, then per job a JobIn followed by S - 1 doubles (z of k = 1 .. S - 1).
// out.bin: per job a smhv_ballistic_clearance_dir.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "smh_ballistics.h"

using namespace smh;

struct JobIn { smhv_weapon w; double d, alt, margin; uint32_t S, pad; };
static_assert(sizeof(JobIn) == 112 && sizeof(smhv_ballistic_clearance_dir) == 96, "the layouts the test packs");

static smhv_ballistic_clearance_dir march(const smhv_weapon_rule &w, double d, double alt, double margin, uint32_t S, const double *z) {
	smhv_ballistic_clearance_dir o;
	memset(&o, 0, sizeof o);
	const double disc = bal_disc(w, d, alt), sq = sqrt(disc), gm = w.g * d, den = 2.0 * w.v2;
	const BalClearArc arc[2] = {bal_clear_arc(w, disc, sq, gm, d, SMHV_ARC_HIGH), bal_clear_arc(w, disc, sq, gm, d, SMHV_ARC_LOW)};
	const bool oor = !(disc >= 0.0), none = d == 0.0;
	uint32_t n_blocked[2] = {0u, 0u}, first[2] = {S, S}, at[2] = {0u, 0u}, n_los = 0u;
	double best[2] = {(double)INFINITY, (double)INFINITY};
	for (uint32_t k = 1u; k < S && !none; ++k) {
		const double t = (double)k / (double)S, x = d * t, gxx = w.g * (x * x);
		if (bal_clear_los(alt, t, z[k - 1u])) ++n_los;
		for (uint32_t a = 0; a < 2u && !oor; ++a) {
			const double m = bal_clear_sample(x, gxx, arc[a].T, arc[a].qq1, den, z[k - 1u]);
			if (m < margin) { ++n_blocked[a]; if (first[a] == S) first[a] = k; }
			if (m < best[a]) { best[a] = m; at[a] = k; }
		}
	}
	uint32_t st[2], bal[2];
	for (uint32_t a = 0; a < 2u; ++a) {
		st[a] = bal_clear_status(oor, none, n_blocked[a] != 0u);
		bal[a] = arc[a].bal;
		o.arc[a].status = st[a]; o.arc[a].first_blocked = first[a]; o.arc[a].n_blocked = n_blocked[a]; o.arc[a].bal = bal[a];
		o.arc[a].min_margin = bal_clear_margin(best[a]); o.arc[a].min_at = at[a];
	}
	o.meters = d; o.alt_delta = alt;
	o.los_blocked = n_los;
	o.valid = 1u;
	o.choice = bal_clear_choice(w.arc, st, bal);
	return o;
}

int main(int argc, char **argv) {
	if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
	FILE *in = fopen(argv[1], "rb");
	if (!in) { perror(argv[1]); return 2; }
	uint32_t n = 0;
	if (fread(&n, 1, 4, in) != 4 || n > 1000000u) { fprintf(stderr, "bad header\n"); return 2; }
	std::vector<smhv_ballistic_clearance_dir> out(n);
	for (uint32_t i = 0; i < n; ++i) {
		JobIn j;
		if (fread(&j, sizeof j, 1, in) != 1 || j.S == 0u || j.S > SMHV_CLEAR_MAX_SAMPLES) { fprintf(stderr, "bad job %u\n", i); return 2; }
		std::vector<double> z(j.S - 1u);
		if (j.S > 1u && fread(z.data(), sizeof(double), j.S - 1u, in) != j.S - 1u) { fprintf(stderr, "short job %u\n", i); return 2; }
		memset(&out[i], 0, sizeof out[i]);
		if (!weapon_ok(&j.w)) continue;
		smhv_weapon_rule rule;
		weapon_rule(&j.w, &rule);
		out[i] = march(rule, j.d, j.alt, j.margin, j.S, z.data());
	}
	fclose(in);
	FILE *f = fopen(argv[2], "wb");
	if (!f) { perror(argv[2]); return 2; }
	if (n && fwrite(out.data(), sizeof out[0], n, f) != n) { fprintf(stderr, "short write\n"); return 2; }
	fclose(f);
	printf("ok: %u jobs\n", n);
	return 0;
}
