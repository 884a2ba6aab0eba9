// smh_maptiles.h -- the rule of the MapTiles message (include/smh_vision_hip.h, "remote-viewer feed: map tiles"): the tile grid of a
// map, a tile's clipped size and padded bytes, the message's length and the choice between MapTiles and Map.  One text for the kernels
// (smh_feedtiles.hip), the host entry points (smh_feedtiles.inc) and a stand-alone host check (tests/map_tiles_check.cpp compiles
// this header with the host compiler), hence SMH_HD.  Integers only.
#pragma once
#include <stdint.h>

#ifndef SMH_HD
#if defined(__HIPCC__)
#define SMH_HD __host__ __device__ __forceinline__
#else
#define SMH_HD static inline
#endif
#endif

namespace smh {

#define SMH_TILE_W 64u                   // pixels: a tile row is 256 bytes of RGBA, one dword per lane of a wave
#define SMH_TILE_H 16u
#define SMH_TILES_HEADER 26u             // bytes in front of the index list: with a message at an offset = 6 (mod 16) the list is 16-byte aligned

struct TileGrid { uint32_t w, h, tiles_x, tiles_y; };

SMH_HD uint64_t tiles_pad16(uint64_t n) { return (n + 15ull) & ~15ull; }
SMH_HD TileGrid tile_grid(uint32_t w, uint32_t h) {
	TileGrid g;
	g.w = w; g.h = h;
	g.tiles_x = (w + SMH_TILE_W - 1u) / SMH_TILE_W; g.tiles_y = (h + SMH_TILE_H - 1u) / SMH_TILE_H;
	return g;
}
SMH_HD uint32_t tile_count(const TileGrid &g) { return g.tiles_x * g.tiles_y; }
// the clipped size of tile t = ty * tiles_x + tx
SMH_HD uint32_t tile_cw(const TileGrid &g, uint32_t tx) { const uint32_t left = g.w - SMH_TILE_W * tx; return left < SMH_TILE_W ? left : SMH_TILE_W; }
SMH_HD uint32_t tile_ch(const TileGrid &g, uint32_t ty) { const uint32_t left = g.h - SMH_TILE_H * ty; return left < SMH_TILE_H ? left : SMH_TILE_H; }
// a tile in the message: ch rows of cw RGBA pixels, tightly packed, then zero bytes up to the next multiple of 16
SMH_HD uint32_t tile_bytes(const TileGrid &g, uint32_t t) {
	const uint32_t ty = t / g.tiles_x, tx = t - ty * g.tiles_x;
	return (uint32_t)tiles_pad16(4ull * tile_cw(g, tx) * tile_ch(g, ty));
}
// L = 26 + pad16(4 n) + the sum of the n tiles' padded bytes
SMH_HD uint64_t tiles_len(uint32_t n, uint64_t tile_bytes_sum) { return SMH_TILES_HEADER + tiles_pad16(4ull * n) + tile_bytes_sum; }
SMH_HD uint64_t tiles_map_len(uint32_t w, uint32_t h) { return 10ull + 4ull * w * h; }
// MapTiles against a base iff L < 10 + 4 w h; every tile changed always gives more, so a wholly new picture goes out as a Map
SMH_HD bool tiles_chosen(uint32_t w, uint32_t h, uint32_t n, uint64_t tile_bytes_sum) { return tiles_len(n, tile_bytes_sum) < tiles_map_len(w, h); }

}  // namespace smh
