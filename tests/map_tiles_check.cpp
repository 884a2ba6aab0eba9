// map_tiles_check.cpp -- csrc/smh_maptiles.h as a stand-alone host program (tests/test_web_tiles_host.py builds it with the host
// compiler, with -fsanitize=address,undefined where that links, and holds its output against tests/web_tiles_ref.py number for
// number).
//   map_tiles_check in.bin out.bin
// in.bin:  u32 jobs, then per job u32 w, h, n and n u32 tile indices.
// out.bin: per job u32 tiles_x, tiles_y, then per tile of the WHOLE grid u32 cw, ch, padded bytes, then u64 L of the n listed tiles,
//          u64 the Map's length, u32 1 where MapTiles is chosen.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "smh_maptiles.h"

using namespace smh;

static bool read_all(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
	if (argc != 3) { fprintf(stderr, "usage: map_tiles_check in.bin out.bin\n"); return 2; }
	FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
	if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
	uint32_t jobs = 0;
	if (!read_all(in, &jobs, 4)) return 2;
	size_t tiles = 0;
	for (uint32_t j = 0; j < jobs; ++j) {
		uint32_t head[3];
		if (!read_all(in, head, sizeof head)) { fprintf(stderr, "job %u: short input\n", j); return 2; }
		std::vector<uint32_t> list(head[2]);
		if (head[2] && !read_all(in, list.data(), 4u * head[2])) { fprintf(stderr, "job %u: short list\n", j); return 2; }
		const TileGrid g = tile_grid(head[0], head[1]);
		const uint32_t dims[2] = {g.tiles_x, g.tiles_y};
		fwrite(dims, sizeof dims, 1, out);
		for (uint32_t t = 0; t < tile_count(g); ++t) {
			const uint32_t row[3] = {tile_cw(g, t % g.tiles_x), tile_ch(g, t / g.tiles_x), tile_bytes(g, t)};
			fwrite(row, sizeof row, 1, out);
			++tiles;
		}
		uint64_t sum = 0;
		for (uint32_t t : list) {
			if (t >= tile_count(g)) { fprintf(stderr, "job %u: tile %u of %u\n", j, t, tile_count(g)); return 2; }
			sum += tile_bytes(g, t);
		}
		const uint64_t lens[2] = {tiles_len(head[2], sum), tiles_map_len(head[0], head[1])};
		const uint32_t chosen = tiles_chosen(head[0], head[1], head[2], sum) ? 1u : 0u;
		fwrite(lens, sizeof lens, 1, out);
		fwrite(&chosen, sizeof chosen, 1, out);
	}
	fclose(in);
	if (fclose(out) != 0) return 2;
	printf("ok: %u jobs, %zu tiles\n", jobs, tiles);
	return 0;
}
