// ballistics_rule_check.cpp -- csrc/smh_ballistics.h as a stand-alone host program (tests/test_ballistics_host.py builds it with the
// host compiler, with -fsanitize=address,undefined where that links, and holds its output against tests/ballistics_ref.py: everything
// bit for bit but the elevations).
//   ballistics_rule_check in.bin out.bin
// in.bin:  u32 jobs, then per job a JobIn.
// out.bin: per job a JobOut.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "smh_ballistics.h"

using namespace smh;

struct JobIn { smhv_weapon w; double m, alt; };
struct JobOut { uint32_t ok, pad; smhv_weapon_rule rule; smhv_ballistic_solution sol; };
static_assert(sizeof(JobIn) == 96 && sizeof(JobOut) == 272, "the layouts the test packs");

int main(int argc, char **argv) {
	if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
	FILE *in = fopen(argv[1], "rb");
	if (!in) { perror(argv[1]); return 2; }
	uint32_t n = 0;
	if (fread(&n, 1, 4, in) != 4 || n > 1000000u) { fprintf(stderr, "bad header\n"); return 2; }
	std::vector<JobIn> jobs(n);
	if (n && fread(jobs.data(), sizeof(JobIn), n, in) != n) { fprintf(stderr, "short input\n"); return 2; }
	fclose(in);
	std::vector<JobOut> out(n);
	for (uint32_t i = 0; i < n; ++i) {
		JobOut &o = out[i];
		memset(&o, 0, sizeof o);
		o.ok = weapon_ok(&jobs[i].w) ? 1u : 0u;
		if (!o.ok) continue;
		weapon_rule(&jobs[i].w, &o.rule);
		o.sol = bal_solve(o.rule, jobs[i].m, jobs[i].alt, 0u);
	}
	FILE *f = fopen(argv[2], "wb");
	if (!f) { perror(argv[2]); return 2; }
	if (n && fwrite(out.data(), sizeof(JobOut), n, f) != n) { fprintf(stderr, "short write\n"); return 2; }
	fclose(f);
	printf("ok: %u jobs\n", n);
	return 0;
}
