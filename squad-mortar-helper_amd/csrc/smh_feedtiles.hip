// smh_feedtiles.hip -- the remote-viewer feed's map tiles (gfx950, wave64): a frame whose ui_map differs from the viewer's texture in a
// few 64 x 16 tiles sends those tiles (the MapTiles message; include/smh_vision_hip.h, "remote-viewer feed: map tiles"; the rule in
// numbers: smh_maptiles.h) in the place of the whole Map.  The reference has no such message.  k_map_crc and k_feed_maps of
// smh_feed.hip run as they are; this file holds what runs between and behind them (smh_kernels.h lists the chain).  No host round
// trip: which frames send tiles, how many, and which frame's map the feed keeps are known on the device only.
#include <hip/hip_runtime.h>

#include "smh_device.h"
#include "smh_maptiles.h"

namespace smh {

static __device__ __forceinline__ bool frame_open(const smhv_frame_result *rec) { return rec->map_open != 0u && rec->status == SMHV_FRAME_OK; }

// inclusive scan over a workgroup of BS threads (Hillis-Steele in LDS; MAX: maximum, else sum); buf: 2 x BS words
template <bool MAX, uint32_t BS>
static __device__ unsigned long long tiles_scan(unsigned long long v, unsigned long long *buf) {
	const uint32_t tid = threadIdx.x;
	uint32_t cur = 0;
	buf[tid] = v;
	__syncthreads();
	for (uint32_t off = 1; off < BS; off <<= 1) {
		unsigned long long x = buf[cur * BS + tid];
		if (tid >= off) {
			const unsigned long long o = buf[cur * BS + tid - off];
			x = MAX ? (o > x ? o : x) : x + o;
		}
		cur ^= 1u;
		buf[cur * BS + tid] = x;
		__syncthreads();
	}
	const unsigned long long out = buf[cur * BS + tid];
	__syncthreads();
	return out;
}

// the kept map is usable iff the feed has a stored CRC, that CRC is the kept map's, and the kept map has this call's size
static __device__ __forceinline__ bool kept_usable(const FeedTilesRun &t) {
	return t.kstate[0] != 0u && t.r.state[0] != 0u && t.r.state[1] == t.kstate[1] && t.kstate[2] == t.r.w && t.kstate[3] == t.r.h;
}

// ------------------------------------------------------------------------------------------------
// k_tiles_base: one workgroup, a thread per frame in chunks of TILES_PLAN_BS; the nearest earlier open frame by a maximum scan
// ------------------------------------------------------------------------------------------------
#define TILES_PLAN_BS 1024u
__global__ void __launch_bounds__(TILES_PLAN_BS) k_tiles_base(FeedTilesRun t) {
	__shared__ unsigned long long buf[2u * TILES_PLAN_BS];
	__shared__ uint32_t carry;                                                            // 1 + the last open frame of the chunks before; 0: none
	const uint32_t tid = threadIdx.x;
	const uint32_t outside = kept_usable(t) ? SMH_TILES_BASE_KEPT : SMH_TILES_BASE_NONE;
	if (tid == 0u) carry = 0u;
	__syncthreads();
	for (uint32_t base = 0; base < t.r.n; base += TILES_PLAN_BS) {
		const uint32_t i = base + tid;
		const bool ok = i < t.r.n && frame_open(t.r.res + min(i, t.r.n - 1u));
		const uint32_t key_incl = (uint32_t)tiles_scan<true, TILES_PLAN_BS>(ok ? i + 1u : 0u, buf);
		buf[tid] = key_incl;
		__syncthreads();
		const uint32_t key_excl = tid ? (uint32_t)buf[tid - 1u] : 0u, before = key_excl ? key_excl : carry;
		if (i < t.r.n) t.base[i] = !ok ? SMH_TILES_BASE_NONE : before ? before - 1u : outside;
		__syncthreads();
		if (tid == TILES_PLAN_BS - 1u && key_incl) carry = key_incl;
		__syncthreads();
	}
}

// ------------------------------------------------------------------------------------------------
// k_tiles_diff, the hot one.  A workgroup takes (frame, 32 consecutive tiles = one word of the frame's bitmap) and leaves at once
// when the frame has no base or its raw CRC equals its base's (equal CRCs count as equal maps).  A wave takes eight of the 32 tiles
// one after the other: a tile row is 64 pixels = one dword per lane, so a lane owns a pixel column of the tile, loads its (up to)
// 16 dwords of both maps -- all in flight together; rows and columns beyond a clipped tile's are clamped onto its last, which
// changes no OR -- and ORs the XORs; one ballot per tile says whether any byte differs (alpha counts).  Both maps are read where
// they lie: a frame's rows in the pitched slab behind the lead-in of xoff pixels, the kept map tightly packed; rows are only 4-byte
// aligned, hence dword loads.  Written: the word's bits and the padded bytes of its set tiles, and per frame the sums (two
// atomicAdds per workgroup).  Nothing the size of a map, no scratch.
// ------------------------------------------------------------------------------------------------
#define TILES_DIFF_BS 256u
__global__ void __launch_bounds__(TILES_DIFF_BS) k_tiles_diff(FeedTilesRun t) {
	__shared__ uint32_t wbits[TILES_DIFF_BS / 64u];
	const FeedRun &r = t.r;
	const uint32_t f = blockIdx.y, wi = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
	const uint32_t b = t.base[f];
	if (b == SMH_TILES_BASE_NONE) return;                                                 // (the whole workgroup; closed and non-OK frames too)
	if (b == SMH_TILES_BASE_KEPT ? (r.raw[f] ^ r.len_term) == t.kstate[1] : r.raw[f] == r.raw[b]) return;
	const TileGrid g = tile_grid(r.w, r.h);
	const uint32_t tiles = tile_count(g);
	const uint32_t *A = (const uint32_t *)(r.ui + (size_t)f * r.ui_stride) + r.xoff;
	const uint32_t pitch_a = (uint32_t)(r.ui_pitch >> 2);
	const uint32_t *B = b == SMH_TILES_BASE_KEPT ? (const uint32_t *)t.kept : (const uint32_t *)(r.ui + (size_t)b * r.ui_stride) + r.xoff;
	const uint32_t pitch_b = b == SMH_TILES_BASE_KEPT ? r.w : pitch_a;
	uint32_t mine = 0u;
	for (uint32_t k = 0; k < 8u; ++k) {
		const uint32_t tl = 32u * wi + 8u * wv + k;
		if (tl >= tiles) break;                                                           // (wave-uniform)
		const uint32_t ty = tl / g.tiles_x, tx = tl - ty * g.tiles_x;
		const uint32_t cw = tile_cw(g, tx), ch = tile_ch(g, ty);
		const uint32_t x = SMH_TILE_W * tx + min(lane, cw - 1u), y0 = SMH_TILE_H * ty;
		uint32_t a[SMH_TILE_H], c[SMH_TILE_H];
#pragma unroll
		for (uint32_t y = 0; y < SMH_TILE_H; ++y) {
			const uint32_t row = y0 + min(y, ch - 1u);                                    // (x < w, row < h: inside both maps)
			a[y] = A[(size_t)row * pitch_a + x];
			c[y] = B[(size_t)row * pitch_b + x];
		}
		uint32_t acc = 0u;
#pragma unroll
		for (uint32_t y = 0; y < SMH_TILE_H; ++y) acc |= a[y] ^ c[y];
		if (__ballot(acc != 0u) != 0ull) mine |= 1u << (8u * wv + k);
	}
	if (lane == 0u) wbits[wv] = mine;
	__syncthreads();
	if (tid == 0u) {
		uint32_t word = 0u, bytes = 0u;
		for (uint32_t k = 0; k < TILES_DIFF_BS / 64u; ++k) word |= wbits[k];
		for (uint32_t m = word; m; m &= m - 1u) bytes += tile_bytes(g, 32u * wi + (uint32_t)__builtin_ctz(m));
		t.bits[(size_t)f * t.words + wi] = make_uint2(word, bytes);
		if (word) { atomicAdd(t.info + 2u * f, (uint32_t)__builtin_popcount(word)); atomicAdd(t.info + 2u * f + 1u, bytes); }
	}
}

// ------------------------------------------------------------------------------------------------
// k_tiles_plan: k_feed_plan (smh_feed.hip) without the snapshot -- the same scans over chunks of 1024 frames with carried state,
// the same capacity cut and frames_done -- where the slot between UpdateState and Markers is, per frame, nothing (the CRC is the
// texture's), a MapTiles message of L bytes (the frame has a base and L < 10 + 4 w h) or the Map.  For a MapTiles message it
// writes the 26 header bytes and an item (k_tiles_copy writes the index list and the tiles), for a Map what k_feed_plan writes;
// and it names the frame whose map the feed keeps: the last consumed open one.
// ------------------------------------------------------------------------------------------------
static __device__ __forceinline__ uint64_t feed_slot(uint64_t len) { return (len + 15ull) & ~15ull; }
static __device__ __forceinline__ void put16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
static __device__ __forceinline__ void put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

__global__ void __launch_bounds__(TILES_PLAN_BS) k_tiles_plan(FeedTilesRun t) {
	__shared__ unsigned long long buf[2u * TILES_PLAN_BS];
	__shared__ uint32_t crc_sh[TILES_PLAN_BS];
	__shared__ uint32_t s_cut;
	__shared__ struct { uint32_t has, crc, entries, maps, tmsgs, done, stop, keep, keep_crc; unsigned long long off, used; } carry;
	const FeedRun &r = t.r;
	const uint32_t tid = threadIdx.x;
	const uint64_t map_len = tiles_map_len(r.w, r.h);
	if (tid == 0u) {
		carry.has = r.state[0]; carry.crc = r.state[1];
		carry.entries = carry.maps = carry.tmsgs = carry.done = carry.stop = 0u;
		carry.keep = SMH_TILES_BASE_NONE; carry.keep_crc = 0u;
		carry.off = 6ull; carry.used = 0ull;
	}
	__syncthreads();
	for (uint32_t base = 0; base < r.n; base += TILES_PLAN_BS) {
		const uint32_t i = base + tid, in_chunk = min(r.n - base, TILES_PLAN_BS);
		const smhv_frame_result *rec = r.res + min(i, r.n - 1u);
		const bool ok = i < r.n && frame_open(rec);
		const uint32_t crc = ok ? (r.raw[i] ^ r.len_term) : 0u;
		if (tid == 0u) s_cut = in_chunk;
		crc_sh[tid] = crc;
		// the CRC the current texture was made from, as frame i finds it: that of the nearest open frame before it, else the carried one
		const uint32_t key_incl = (uint32_t)tiles_scan<true, TILES_PLAN_BS>(ok ? tid + 1u : 0u, buf);
		buf[tid] = key_incl;
		__syncthreads();
		const uint32_t key_excl = tid ? (uint32_t)buf[tid - 1u] : 0u;
		const uint32_t prev_has = key_excl ? 1u : carry.has, prev_crc = key_excl ? crc_sh[key_excl - 1u] : carry.crc;
		__syncthreads();
		// the frame's messages: UpdateState, MapTiles or Map, Markers
		const uint32_t n_lines = ok ? min(rec->n_lines, (uint32_t)SMHV_MAX_LINES) : 0u;
		const uint32_t len_u = ok && rec->has_minimap ? 27u : 11u, len_k = 7u + 16u * n_lines;
		const bool pm = ok && (!prev_has || crc != prev_crc);
		const uint32_t n_tiles = pm ? t.info[2u * min(i, r.n - 1u)] : 0u, tile_sum = pm ? t.info[2u * min(i, r.n - 1u) + 1u] : 0u;
		const bool pt = pm && t.base[i] != SMH_TILES_BASE_NONE && tiles_chosen(r.w, r.h, n_tiles, tile_sum);   // (a base implies prev_has, and prev_crc is the base's CRC)
		const uint64_t mlen = pt ? tiles_len(n_tiles, tile_sum) : map_len;
		const uint32_t nmsg = ok ? 2u + (uint32_t)pm : 0u;
		const uint64_t size = ok ? feed_slot(len_u) + (pm ? feed_slot(mlen) : 0ull) + feed_slot(len_k) : 0ull;
		const uint64_t size_incl = tiles_scan<false, TILES_PLAN_BS>(size, buf);
		const uint64_t off = carry.off + (size_incl - size);
		const uint64_t end = off + size - (feed_slot(len_k) - len_k);                      // where the frame's last message (Markers) ends
		if (nmsg && end > r.capacity) atomicMin(&s_cut, tid);
		// messages, Maps and MapTiles messages before this frame: 21 bits each (a call has at most 65535 frames)
		const unsigned long long cnt_incl =
			tiles_scan<false, TILES_PLAN_BS>((unsigned long long)nmsg | ((unsigned long long)(pm && !pt) << 21) | ((unsigned long long)pt << 42), buf);
		const uint32_t cut = s_cut;                                                        // frames of this chunk that are consumed
		buf[tid] = end;
		if (tid < cut && nmsg) {
			uint32_t e = carry.entries + (uint32_t)(cnt_incl & 0x1FFFFFu) - nmsg;
			const uint32_t mi = carry.maps + (uint32_t)((cnt_incl >> 21) & 0x1FFFFFu) - (uint32_t)(pm && !pt);
			const uint32_t ti = carry.tmsgs + (uint32_t)(cnt_incl >> 42) - (uint32_t)pt;
			uint64_t o = off;
			smhv_feed_entry en;
			en.frame = r.first + i; en.crc = crc;
			{
				uint8_t *p = r.bytes + o;
				const unsigned long long bits = rec->has_mpx ? (unsigned long long)__double_as_longlong(rec->mpx) : 0ull;   // unwrap_or(0.0)
				put16(p, SMHV_WEB_UPDATE_STATE);
				put32(p + 2, (uint32_t)bits); put32(p + 6, (uint32_t)(bits >> 32));
				p[10] = rec->has_minimap ? 1u : 0u;
				if (rec->has_minimap)
					for (uint32_t k = 0; k < 4u; ++k) put32(p + 11u + 4u * k, rec->minimap[k]);
				en.offset = o; en.length = len_u; en.kind = SMHV_WEB_UPDATE_STATE;
				r.entries[e++] = en;
				o += feed_slot(len_u);
			}
			if (pm) {
				uint8_t *p = r.bytes + o;
				if (pt) {
					put16(p, SMHV_WEB_MAP_TILES); put32(p + 2, r.w); put32(p + 6, r.h);
					put16(p + 10, SMH_TILE_W); put16(p + 12, SMH_TILE_H);
					put32(p + 14, n_tiles); put32(p + 18, prev_crc); put32(p + 22, crc);
					t.items[ti].dst = o; t.items[ti].frame = i; t.items[ti].n = n_tiles;
				} else {
					put16(p, SMHV_WEB_MAP); put32(p + 2, r.w); put32(p + 6, r.h);
					r.maps[mi].dst = o + 10ull; r.maps[mi].frame = i; r.maps[mi].pad = 0u;
				}
				en.offset = o; en.length = (uint32_t)mlen; en.kind = pt ? SMHV_WEB_MAP_TILES : SMHV_WEB_MAP;
				r.entries[e++] = en;
				o += feed_slot(mlen);
			}
			{
				uint8_t *p = r.bytes + o;
				put16(p, SMHV_WEB_MARKERS);
				p[2] = 0u;
				put32(p + 3, n_lines);
				const uint32_t *src = (const uint32_t *)rec->lines;                             // bit for bit (NaN payloads included)
				for (uint32_t k = 0; k < 4u * n_lines; ++k) put32(p + 7u + 4u * k, src[k]);
				en.offset = o; en.length = len_k; en.kind = SMHV_WEB_MARKERS;
				r.entries[e++] = en;
			}
		}
		__syncthreads();                                                                      // (everybody has read the carried state)
		if (cut && tid == cut - 1u) {                                                         // the chunk's last consumed frame carries it on
			carry.off += size_incl;
			carry.entries += (uint32_t)(cnt_incl & 0x1FFFFFu); carry.maps += (uint32_t)((cnt_incl >> 21) & 0x1FFFFFu); carry.tmsgs += (uint32_t)(cnt_incl >> 42);
			if (key_incl) {
				carry.has = 1u; carry.crc = crc_sh[key_incl - 1u];
				carry.used = buf[key_incl - 1u];                                              // the end of the last consumed open frame
				carry.keep = base + key_incl - 1u; carry.keep_crc = crc_sh[key_incl - 1u];
			}
			carry.done = base + cut;
		}
		if (tid == 0u) carry.stop = cut < in_chunk;
		__syncthreads();
		if (carry.stop) break;
	}
	if (tid == 0u) {
		smhv_feed_header h;
		h.n_entries = carry.entries; h.frames_done = carry.done; h.n_maps = carry.maps;
		h.has_last_crc = carry.has; h.last_crc = carry.crc; h.reserved = 0u; h.bytes_used = carry.used;
		*r.header = h;
		r.state[0] = carry.has; r.state[1] = carry.crc;
		t.ctl[0] = carry.tmsgs; t.ctl[1] = carry.keep; t.ctl[2] = carry.keep_crc;
	}
}

// ------------------------------------------------------------------------------------------------
// k_tiles_copy: the index lists and the tiles.  How many MapTiles messages there are is known on the device only, so a fixed grid of
// persistent workgroups walks the (message, bitmap word) items and leaves at once when there is none.  For its word the workgroup
// sums the set bits and the padded bytes of the words before it (a reduction over the frame's words: the prefix count the
// destination comes from), then takes the word's set tiles one by one: a lane owns 16 consecutive bytes of the padded tile -- a
// tile is at most 256 such groups, the workgroup's width -- finds its four dwords in (row, column) of the clipped tile, loads them
// from the slab (zero beyond the tile's last pixel: the padding, written explicitly) and stores them as one aligned 16-byte store.
// The list's entry is one dword store; the list's padding is written with the message's first word.
// ------------------------------------------------------------------------------------------------
#define TILES_COPY_BS 256u
__global__ void __launch_bounds__(TILES_COPY_BS) k_tiles_copy(FeedTilesRun t) {
	__shared__ uint32_t red[2][TILES_COPY_BS / 64u];
	const FeedRun &r = t.r;
	const uint32_t n_msgs = t.ctl[0];
	if (!n_msgs) return;
	const TileGrid g = tile_grid(r.w, r.h);
	const uint64_t items = (uint64_t)n_msgs * t.words;
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
	const uint32_t pitch_dw = (uint32_t)(r.ui_pitch >> 2);
	for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
		const uint32_t m = (uint32_t)(item / t.words), wi = (uint32_t)(item - (uint64_t)m * t.words);
		const FeedTileItem it = t.items[m];
		const uint2 *fb = t.bits + (size_t)it.frame * t.words;
		const uint32_t word = fb[wi].x;
		if (!word && wi) continue;                                                        // (the whole workgroup)
		uint32_t cnt = 0u, bytes = 0u;
		for (uint32_t j = tid; j < wi; j += TILES_COPY_BS) { const uint2 v = fb[j]; cnt += (uint32_t)__builtin_popcount(v.x); bytes += v.y; }
		cnt = wave_sum32(cnt); bytes = wave_sum32(bytes);
		__syncthreads();                                                                  // (the previous item's sums have been read)
		if (lane == 0u) { red[0][wv] = cnt; red[1][wv] = bytes; }
		__syncthreads();
		cnt = bytes = 0u;
		for (uint32_t k = 0; k < TILES_COPY_BS / 64u; ++k) { cnt += red[0][k]; bytes += red[1][k]; }
		uint32_t *list = (uint32_t *)(r.bytes + it.dst + SMH_TILES_HEADER);               // (16-byte aligned: dst = 6 (mod 16))
		uint8_t *tiles_at = (uint8_t *)list + tiles_pad16(4ull * it.n);
		if (wi == 0u && tid < ((0u - it.n) & 3u)) list[it.n + tid] = 0u;                  // zero bytes up to a multiple of 16
		const uint32_t *src = (const uint32_t *)(r.ui + (size_t)it.frame * r.ui_stride) + r.xoff;
		for (uint32_t mk = word; mk; mk &= mk - 1u) {
			const uint32_t tl = 32u * wi + (uint32_t)__builtin_ctz(mk);
			const uint32_t ty = tl / g.tiles_x, tx = tl - ty * g.tiles_x;
			const uint32_t cw = tile_cw(g, tx), ch = tile_ch(g, ty), dwords = cw * ch, tb = tile_bytes(g, tl);
			if (tid == 0u) list[cnt] = tl;
			if (16u * tid < tb) {
				uint32_t q = 4u * tid, row = q / cw, col = q - row * cw;                   // (q < dwords: 16 tid < pad16(4 dwords))
				uint32_t d[4];
#pragma unroll
				for (uint32_t k = 0; k < 4u; ++k) {
					d[k] = q < dwords ? src[(size_t)(SMH_TILE_H * ty + row) * pitch_dw + SMH_TILE_W * tx + col] : 0u;
					++q; if (++col == cw) { col = 0u; ++row; }
				}
				*(uint4 *)(tiles_at + bytes + 16u * tid) = make_uint4(d[0], d[1], d[2], d[3]);
			}
			++cnt; bytes += tb;
		}
	}
}

// ------------------------------------------------------------------------------------------------
// k_tiles_keep: the last consumed open frame's map, tightly packed, and its CRC into the feed (the plan named the frame; a call that
// consumed none leaves the kept map as it is).  Destination driven like k_feed_maps: a lane owns 16 bytes of the kept map.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_tiles_keep(FeedTilesRun t) {
	const FeedRun &r = t.r;
	const uint32_t f = t.ctl[1];
	if (f == SMH_TILES_BASE_NONE) return;
	const uint32_t dwords = r.w * r.h, groups = (dwords + 3u) >> 2, pitch_dw = (uint32_t)(r.ui_pitch >> 2);
	const uint32_t *src = (const uint32_t *)(r.ui + (size_t)f * r.ui_stride) + r.xoff;
	for (uint32_t gi = blockIdx.x * 256u + threadIdx.x; gi < groups; gi += gridDim.x * 256u) {
		uint32_t q = 4u * gi, row = q / r.w, col = q - row * r.w;
		uint32_t d[4];
#pragma unroll
		for (uint32_t k = 0; k < 4u; ++k) {
			d[k] = q < dwords ? src[(size_t)row * pitch_dw + col] : 0u;
			++q; if (++col == r.w) { col = 0u; ++row; }
		}
		*(uint4 *)(t.kept + 16ull * gi) = make_uint4(d[0], d[1], d[2], d[3]);                 // (the kept map's buffer is a multiple of 16 bytes)
	}
	if (blockIdx.x == 0u && threadIdx.x == 0u) { t.kstate[0] = 1u; t.kstate[1] = t.ctl[2]; t.kstate[2] = r.w; t.kstate[3] = r.h; }
}

// ------------------------------------------------------------------------------------------------
// launcher
// ------------------------------------------------------------------------------------------------
hipError_t launch_feed_tiles(const FeedTilesRun &t, hipStream_t s) {
	const FeedRun &r = t.r;
	hipError_t e = hipMemsetAsync(r.raw, 0, sizeof(uint32_t) * r.n, s);
	if (e == hipSuccess) e = hipMemsetAsync(t.info, 0, sizeof(uint32_t) * 2u * r.n, s);
	if (e != hipSuccess) return e;
	const uint32_t band = 4u * r.rows_per_wave;                                               // (k_map_crc: four waves per workgroup)
	hipLaunchKernelGGL(k_map_crc, dim3((r.h + band - 1u) / band, r.n), dim3(256), 0, s, r);
	hipLaunchKernelGGL(k_tiles_base, dim3(1), dim3(TILES_PLAN_BS), 0, s, t);
	hipLaunchKernelGGL(k_tiles_diff, dim3(t.words, r.n), dim3(TILES_DIFF_BS), 0, s, t);
	hipLaunchKernelGGL(k_tiles_plan, dim3(1), dim3(TILES_PLAN_BS), 0, s, t);
	hipLaunchKernelGGL(k_tiles_copy, dim3(2048), dim3(TILES_COPY_BS), 0, s, t);
	hipLaunchKernelGGL(k_feed_maps, dim3(2048), dim3(256), 0, s, r);
	hipLaunchKernelGGL(k_tiles_keep, dim3(512), dim3(256), 0, s, t);
	return hipGetLastError();
}

}  // namespace smh
