// smh_feed.hip -- the remote-viewer feed (gfx950, wave64): the web server's events of every processed frame, written on the
// device (include/smh_vision_hip.h, "remote-viewer feed"; reference web/src/lib.rs:127-214, src/ui/state.rs:81-88,
// src/ui/map.rs:213-233).  Three kernels per call, chained on one stream with no host round trip:
//   k_map_crc     CRC-32 of every open frame's ui_map, read where it lies in the pitched ui slab
//   k_feed_plan   one workgroup: the "changed since the last texture" rule in frame order, message sizes and offsets, the
//                 capacity cut, header, entries, the new stored CRC, and the bytes of the small messages
//   k_feed_maps   the Map payloads: pitched rows -> tight, 16-byte aligned payloads, for the frames the plan gave a Map entry
// and k_feed_tables, which a feed runs once per map geometry (the powers of x the CRC needs).  With a debug view as the Map
// (smhv_batch_feed_view) the first and the third are k_view_crc / k_view_crc_gray1 and k_feed_view_maps further down: the same
// structure over a message generated from its source; these four stay as they are.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "smh_device.h"

namespace smh {

// x^n mod P (reflected representation, x^0 = 0x80000000)
static __device__ uint32_t xpow(uint64_t n) {
	uint32_t r = 0x80000000u, b = 0x40000000u;
	for (; n; n >>= 1) { if (n & 1u) r = gf2_mulmod(r, b); b = gf2_mulmod(b, b); }
	return r;
}

// tab[c], c < quads: x^(32 * dwords of a row behind the last map dword of the row's 16-byte group c)   (align a group to its row's end)
// tab[quads + k], k < h: x^(32 w k)                                                                     (align a row to the map's end)
__global__ void __launch_bounds__(256) k_feed_tables(uint32_t *tab, uint32_t w, uint32_t h, uint32_t xoff, uint32_t quads) {
	const uint32_t t = blockIdx.x * 256u + threadIdx.x;
	if (t < quads) {
		const uint32_t last = min(4u * t + 3u - xoff, w - 1u);       // (xoff <= 3)
		tab[t] = xpow(32ull * (w - 1u - last));
	} else if (t < quads + h)
		tab[t] = xpow(32ull * w * (uint64_t)(t - quads));
}

// ------------------------------------------------------------------------------------------------
// k_map_crc.  The message of a frame is its h rows of 4 w bytes, concatenated; pitch padding and the lead-in of `xoff`
// pixels are not part of it.  CRC without init / final xor is linear over GF(2):
//     R(message) = XOR_y R(row y) * x^(32 w (h - 1 - y)) mod P
// A workgroup takes (frame, band of rows), a wave a run of the band's rows, and a lane the same K consecutive 16-byte groups of
// every row of its wave: it folds them with the slice-by-4 step (tables in LDS, as k_crc32 has them) starting from 0 -- leading
// zeros do not change R, so the lead-in costs nothing and the loads are the slab's own aligned 16-byte groups; dwords beyond
// the row's end are skipped -- and carries its remainder from row to row by Horner's rule, acc = acc * x^(32 w) ^ v, where the
// multiplication by that one constant is four more lookups (mrow[k][b] = (b << 8 k) * x^(32 w)).  At the end one generic
// multiplication per lane aligns its groups to the row's end, an xor reduction joins the lanes, one multiplication per wave
// aligns its last row to the map's end, and the workgroup issues one atomicXor into the frame's word.  The init / final-xor
// term depends on w h only and is applied by the plan.  One read of the map's bytes; one LDS lookup per byte.
// ------------------------------------------------------------------------------------------------
#define FEED_CRC_BS 256u
__global__ void __launch_bounds__(FEED_CRC_BS) k_map_crc(FeedRun r) {
	__shared__ uint32_t tab[4][256], mrow[4][256], wsum[FEED_CRC_BS / 64u];
	const uint32_t f = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
	if (!r.res[f].map_open || r.res[f].status != SMHV_FRAME_OK) return;        // (the whole workgroup: such a frame has no ui_map)
	{
		uint32_t c = tid;
		for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? SMH_CRC_POLY : 0u);
		tab[0][tid] = c;
		const uint32_t xrow = r.tab[r.quads + 1u];                               // x^(32 w)
#pragma unroll
		for (uint32_t k = 0; k < 4u; ++k) mrow[k][tid] = gf2_mulmod(tid << (8u * k), xrow);
	}
	__syncthreads();
	{
		uint32_t c = tab[0][tid];
		for (int k = 1; k < 4; ++k) { c = (c >> 8) ^ tab[0][c & 255u]; tab[k][tid] = c; }
	}
	__syncthreads();
	const uint32_t K = (r.quads + 63u) >> 6;                                      // 16-byte groups per lane and row
	const uint32_t c0 = min(lane * K, r.quads), c1 = min(c0 + K, r.quads);
	const uint32_t y0 = min((blockIdx.x * (FEED_CRC_BS / 64u) + wv) * r.rows_per_wave, r.h), y1 = min(y0 + r.rows_per_wave, r.h);
	const uint8_t *frame = r.ui + (size_t)f * r.ui_stride;
	const int32_t xoff = (int32_t)r.xoff, w = (int32_t)r.w;
	uint32_t acc = 0;
	for (uint32_t y = y0; y < y1; ++y) {
		const uint4 *row = (const uint4 *)(frame + (size_t)y * r.ui_pitch);      // (16-byte aligned: the pitch is a multiple of 16)
		uint32_t v = 0;
		for (uint32_t cb = c0; cb < c1; cb += 4u) {
			uint4 q[4];
#pragma unroll
			for (uint32_t u = 0; u < 4u; ++u) q[u] = row[min(cb + u, c1 - 1u)];   // four loads in flight; the clamp keeps them inside the lane's groups
#pragma unroll
			for (uint32_t u = 0; u < 4u; ++u) {
				if (cb + u >= c1) break;
				const uint32_t d[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
				const int32_t j0 = (int32_t)(4u * (cb + u)) - xoff;                // map dword of the group's first dword
#pragma unroll
				for (int i = 0; i < 4; ++i) {
					if (j0 + i < 0 || j0 + i >= w) continue;
					const uint32_t c = v ^ d[i];
					v = tab[3][c & 255u] ^ tab[2][(c >> 8) & 255u] ^ tab[1][(c >> 16) & 255u] ^ tab[0][c >> 24];
				}
			}
		}
		acc = mrow[0][acc & 255u] ^ mrow[1][(acc >> 8) & 255u] ^ mrow[2][(acc >> 16) & 255u] ^ mrow[3][acc >> 24] ^ v;
	}
	if (c0 < c1 && y0 < y1) acc = gf2_mulmod(acc, r.tab[c1 - 1u]); else acc = 0u;
	acc = wave_xor32_dpp(acc);
	if (lane == 0u) wsum[wv] = y0 < y1 ? gf2_mulmod(acc, r.tab[r.quads + (r.h - y1)]) : 0u;
	__syncthreads();
	if (tid == 0u) {
		uint32_t x = 0;
		for (uint32_t k = 0; k < FEED_CRC_BS / 64u; ++k) x ^= wsum[k];
		atomicXor(r.raw + f, x);
	}
}

// ------------------------------------------------------------------------------------------------
// k_feed_plan: one workgroup, a thread per frame (frames in chunks of FEED_PLAN_BS, state carried from chunk to chunk).
// ------------------------------------------------------------------------------------------------
#define FEED_PLAN_BS 1024u

// inclusive scan over the workgroup (Hillis-Steele in LDS; MAX: maximum, else sum); buf: 2 x FEED_PLAN_BS words
template <bool MAX>
static __device__ unsigned long long plan_scan(unsigned long long v, unsigned long long *buf) {
	const uint32_t tid = threadIdx.x;
	uint32_t cur = 0;
	buf[tid] = v;
	__syncthreads();
	for (uint32_t off = 1; off < FEED_PLAN_BS; off <<= 1) {
		unsigned long long x = buf[cur * FEED_PLAN_BS + tid];
		if (tid >= off) {
			const unsigned long long o = buf[cur * FEED_PLAN_BS + tid - off];
			x = MAX ? (o > x ? o : x) : x + o;
		}
		cur ^= 1u;
		buf[cur * FEED_PLAN_BS + tid] = x;
		__syncthreads();
	}
	const unsigned long long out = buf[cur * FEED_PLAN_BS + tid];
	__syncthreads();
	return out;
}

// messages start at offsets = 6 (mod 16): a message of `len` bytes takes this much of the buffer
static __device__ __forceinline__ uint64_t feed_slot(uint64_t len) { return (len + 15ull) & ~15ull; }

// little-endian stores at any alignment (a message's fields sit at odd offsets)
static __device__ __forceinline__ void put16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
static __device__ __forceinline__ void put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

__global__ void __launch_bounds__(FEED_PLAN_BS) k_feed_plan(FeedRun r) {
	__shared__ unsigned long long buf[2u * FEED_PLAN_BS];
	__shared__ uint32_t crc_sh[FEED_PLAN_BS];
	__shared__ uint32_t s_cut;
	__shared__ struct { uint32_t has, crc, entries, maps, done, stop; unsigned long long off, used; } carry;
	const uint32_t tid = threadIdx.x;
	const bool snapshot = (r.flags & SMHV_FEED_SNAPSHOT) != 0u;
	const uint64_t map_len = 10ull + (uint64_t)r.w * r.h * 4u;
	if (tid == 0u) {
		carry.has = r.state[0]; carry.crc = r.state[1];
		carry.entries = carry.maps = carry.done = carry.stop = 0u;
		carry.off = 6ull; carry.used = 0ull;
	}
	__syncthreads();
	for (uint32_t base = 0; base < r.n; base += FEED_PLAN_BS) {
		const uint32_t i = base + tid, in_chunk = min(r.n - base, FEED_PLAN_BS);
		const smhv_frame_result *rec = r.res + min(i, r.n - 1u);
		const bool ok = i < r.n && rec->map_open != 0u && rec->status == SMHV_FRAME_OK;
		const uint32_t crc = ok ? (r.raw[i] ^ r.len_term) : 0u;
		if (tid == 0u) s_cut = in_chunk;
		crc_sh[tid] = crc;
		// the CRC the current texture was made from, as frame i finds it: that of the nearest open frame before it, else the carried one
		const uint32_t key_incl = (uint32_t)plan_scan<true>(ok ? tid + 1u : 0u, buf);
		buf[tid] = key_incl;
		__syncthreads();
		const uint32_t key_excl = tid ? (uint32_t)buf[tid - 1u] : 0u;
		const uint32_t prev_has = key_excl ? 1u : carry.has, prev_crc = key_excl ? crc_sh[key_excl - 1u] : carry.crc;
		__syncthreads();
		// the frame's messages: UpdateState, Map, Markers (a snapshot: Map, UpdateState, Markers)
		const uint32_t n_lines = ok ? min(rec->n_lines, (uint32_t)SMHV_MAX_LINES) : 0u;
		const uint32_t len_u = ok && rec->has_minimap ? 27u : 11u, len_k = 7u + 16u * n_lines;
		const bool pu = ok && (!snapshot || rec->has_mpx || rec->has_minimap);
		const bool pm = ok && (snapshot || !prev_has || crc != prev_crc);
		const bool pk = ok && (!snapshot || n_lines != 0u);
		const uint32_t nmsg = (uint32_t)pu + (uint32_t)pm + (uint32_t)pk;
		const uint64_t size = (pu ? feed_slot(len_u) : 0ull) + (pm ? feed_slot(map_len) : 0ull) + (pk ? feed_slot(len_k) : 0ull);
		const uint64_t last_len = pk ? len_k : (pu ? len_u : map_len);                       // (Markers is last in both orders, UpdateState before it)
		const uint64_t size_incl = plan_scan<false>(size, buf);
		const uint64_t off = carry.off + (size_incl - size);
		const uint64_t end = off + size - (feed_slot(last_len) - last_len);                   // where the frame's last message ends
		if (nmsg && end > r.capacity) atomicMin(&s_cut, tid);
		const unsigned long long cnt_incl = plan_scan<false>((unsigned long long)nmsg | ((unsigned long long)pm << 32), buf);
		const uint32_t cut = s_cut;                                                           // frames of this chunk that are consumed
		buf[tid] = end;
		if (tid < cut && nmsg) {
			uint32_t e = carry.entries + (uint32_t)cnt_incl - nmsg;
			const uint32_t mi = carry.maps + (uint32_t)(cnt_incl >> 32) - (uint32_t)pm;
			uint64_t o = off;
			smhv_feed_entry en;
			en.frame = r.first + i; en.crc = crc;
			if (pm && snapshot) {
				uint8_t *p = r.bytes + o;
				put16(p, SMHV_WEB_MAP); put32(p + 2, r.w); put32(p + 6, r.h);
				r.maps[mi].dst = o + 10ull; r.maps[mi].frame = i; r.maps[mi].pad = 0u;
				en.offset = o; en.length = (uint32_t)map_len; en.kind = SMHV_WEB_MAP;
				r.entries[e++] = en;
				o += feed_slot(map_len);
			}
			if (pu) {
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
			if (pm && !snapshot) {
				uint8_t *p = r.bytes + o;
				put16(p, SMHV_WEB_MAP); put32(p + 2, r.w); put32(p + 6, r.h);
				r.maps[mi].dst = o + 10ull; r.maps[mi].frame = i; r.maps[mi].pad = 0u;
				en.offset = o; en.length = (uint32_t)map_len; en.kind = SMHV_WEB_MAP;
				r.entries[e++] = en;
				o += feed_slot(map_len);
			}
			if (pk) {
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
			carry.entries += (uint32_t)cnt_incl; carry.maps += (uint32_t)(cnt_incl >> 32);
			if (key_incl && !snapshot) { carry.has = 1u; carry.crc = crc_sh[key_incl - 1u]; }
			if (key_incl) carry.used = buf[key_incl - 1u];                                    // the end of the last consumed frame that has messages (every open frame has)
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
	}
}

// ------------------------------------------------------------------------------------------------
// k_feed_maps: the Map payloads.  How many there are is known on the device only (the header the plan wrote), so a fixed grid of
// persistent workgroups walks the (map, block of 16-byte groups) items and leaves at once when there is none.  Destination
// driven: a lane owns 16 consecutive payload bytes (the payloads are 16-byte aligned), finds them in (row, column) and loads the
// four source dwords -- rows are only 4-byte aligned in the slab, and a group may straddle a row's end.
// ------------------------------------------------------------------------------------------------
#define FEED_COPY_BS 256u
#define FEED_COPY_GROUPS 4u                      // 16-byte groups per lane and item
__global__ void __launch_bounds__(FEED_COPY_BS) k_feed_maps(FeedRun r) {
	const uint32_t n_maps = r.header->n_maps;
	if (!n_maps) return;
	const uint32_t dwords = r.w * r.h;                                                       // (w <= 4096, h <= 16384)
	const uint32_t groups = (dwords + 3u) >> 2, per_item = FEED_COPY_BS * FEED_COPY_GROUPS;
	const uint32_t items_per_map = (groups + per_item - 1u) / per_item;
	const uint64_t items = (uint64_t)n_maps * items_per_map;
	const uint32_t pitch_dw = (uint32_t)(r.ui_pitch >> 2);
	for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
		const uint32_t m = (uint32_t)(item / items_per_map), ib = (uint32_t)(item - (uint64_t)m * items_per_map);
		const FeedMap fm = r.maps[m];
		const uint32_t *src = (const uint32_t *)(r.ui + (size_t)fm.frame * r.ui_stride) + r.xoff;
		uint8_t *dst = r.bytes + fm.dst;
		uint32_t d[FEED_COPY_GROUPS][4];
#pragma unroll
		for (uint32_t u = 0; u < FEED_COPY_GROUPS; ++u) {
			const uint32_t g = ib * per_item + u * FEED_COPY_BS + threadIdx.x;
			uint32_t q = min(4u * g, dwords - 1u), row = q / r.w, col = q - row * r.w;
#pragma unroll
			for (uint32_t k = 0; k < 4u; ++k) {
				d[u][k] = src[(size_t)row * pitch_dw + col];                                   // (clamped to the map's last dword: always inside the frame)
				if (q + 1u < dwords) { ++q; if (++col == r.w) { col = 0u; ++row; } }
			}
		}
#pragma unroll
		for (uint32_t u = 0; u < FEED_COPY_GROUPS; ++u) {
			const uint32_t g = ib * per_item + u * FEED_COPY_BS + threadIdx.x;
			if (g >= groups) continue;
			if (4u * g + 4u <= dwords) *(uint4 *)(dst + 16ull * g) = make_uint4(d[u][0], d[u][1], d[u][2], d[u][3]);
			else
				for (uint32_t k = 0; 4u * g + k < dwords; ++k) *(uint32_t *)(dst + 16ull * g + 4u * k) = d[u][k];
		}
	}
}

// ------------------------------------------------------------------------------------------------
// A debug view as the Map (smhv_batch_feed_view): the message no longer lies in memory -- its RGBA bytes are generated from a plane
// of one byte per pixel (SMH_RND_SRC_GRAY: the ocr, scales or mask slab), from the colour ui slab through the marker predicate
// (SMH_RND_SRC_PREPROCESS) or from the slab's bottom right quarter (SMH_RND_SRC_CROPPED), exactly the bytes k_render_map_layers
// samples for that source.  The kernels below are k_map_crc and k_feed_maps over a FeedRun whose ui / ui_pitch / ui_stride / w / h /
// xoff / quads describe the SOURCE: for the colour sources the ui slab (CROPPED: advanced by rh / 2 rows and by the whole 16-byte
// groups of m_xoff + rw / 2 pixels, xoff the residual of at most 3 pixels, w x h the quarter's), for a plane its rows, xoff the
// bytes in front of a row's first pixel and `quads` its 16-byte groups of SIXTEEN pixels.  k_feed_plan takes the same FeedRun as it is.
// ------------------------------------------------------------------------------------------------
template <uint32_t SRC>
static __device__ __forceinline__ uint32_t view_px(uint32_t p) {      // a colour source's message dword from the slab's
	if (SRC == SMH_RND_SRC_CROPPED) return p | 0xFF000000u;
	return is_marker(p & 255u, (p >> 8) & 255u, (p >> 16) & 255u) ? (p | 0xFF000000u) : 0xFF000000u;
}
static __device__ __forceinline__ uint32_t view_gray(uint32_t l) { return l * 0x00010101u | 0xFF000000u; }

// k_feed_tables with `ppg` message dwords per 16-byte source group (16 for a plane)
__global__ void __launch_bounds__(256) k_feed_view_tables(uint32_t *tab, uint32_t w, uint32_t h, uint32_t xoff, uint32_t quads, uint32_t ppg) {
	const uint32_t t = blockIdx.x * 256u + threadIdx.x;
	if (t < quads) {
		const uint32_t last = min(ppg * t + (ppg - 1u) - xoff, w - 1u);   // (xoff < ppg)
		tab[t] = xpow(32ull * (w - 1u - last));
	} else if (t < quads + h)
		tab[t] = xpow(32ull * w * (uint64_t)(t - quads));
}

// k_map_crc over a generated message: the same bands, Horner step, alignments and atomicXor; a group's dwords are made from what
// was loaded before they are folded.  A plane's group yields sixteen dwords, so there the LDS lookups decide, not the loads.
template <uint32_t SRC>
__global__ void __launch_bounds__(FEED_CRC_BS) k_view_crc(FeedRun r) {
	constexpr uint32_t PPG = SRC == SMH_RND_SRC_GRAY ? 16u : 4u;
	__shared__ uint32_t tab[4][256], mrow[4][256], wsum[FEED_CRC_BS / 64u];
	const uint32_t f = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
	if (!r.res[f].map_open || r.res[f].status != SMHV_FRAME_OK) return;
	{
		uint32_t c = tid;
		for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? SMH_CRC_POLY : 0u);
		tab[0][tid] = c;
		const uint32_t xrow = r.tab[r.quads + 1u];                               // x^(32 w)
#pragma unroll
		for (uint32_t k = 0; k < 4u; ++k) mrow[k][tid] = gf2_mulmod(tid << (8u * k), xrow);
	}
	__syncthreads();
	{
		uint32_t c = tab[0][tid];
		for (int k = 1; k < 4; ++k) { c = (c >> 8) ^ tab[0][c & 255u]; tab[k][tid] = c; }
	}
	__syncthreads();
	const uint32_t K = (r.quads + 63u) >> 6;
	const uint32_t c0 = min(lane * K, r.quads), c1 = min(c0 + K, r.quads);
	const uint32_t y0 = min((blockIdx.x * (FEED_CRC_BS / 64u) + wv) * r.rows_per_wave, r.h), y1 = min(y0 + r.rows_per_wave, r.h);
	const uint8_t *frame = r.ui + (size_t)f * r.ui_stride;
	const int32_t xoff = (int32_t)r.xoff, w = (int32_t)r.w;
	uint32_t acc = 0;
	for (uint32_t y = y0; y < y1; ++y) {
		const uint4 *row = (const uint4 *)(frame + (size_t)y * r.ui_pitch);      // (16-byte aligned: pitch and base are multiples of 16)
		uint32_t v = 0;
		for (uint32_t cb = c0; cb < c1; cb += 4u) {
			uint4 q[4];
#pragma unroll
			for (uint32_t u = 0; u < 4u; ++u) q[u] = row[min(cb + u, c1 - 1u)];
#pragma unroll
			for (uint32_t u = 0; u < 4u; ++u) {
				if (cb + u >= c1) break;
				const uint32_t d[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
				const int32_t j0 = (int32_t)(PPG * (cb + u)) - xoff;                // message dword of the group's first pixel
#pragma unroll
				for (uint32_t i = 0; i < PPG; ++i) {
					if (j0 + (int32_t)i < 0 || j0 + (int32_t)i >= w) continue;
					const uint32_t m = SRC == SMH_RND_SRC_GRAY ? view_gray((d[i >> 2] >> (8u * (i & 3u))) & 255u) : view_px<SRC>(d[i & 3u]);
					const uint32_t c = v ^ m;
					v = tab[3][c & 255u] ^ tab[2][(c >> 8) & 255u] ^ tab[1][(c >> 16) & 255u] ^ tab[0][c >> 24];
				}
			}
		}
		acc = mrow[0][acc & 255u] ^ mrow[1][(acc >> 8) & 255u] ^ mrow[2][(acc >> 16) & 255u] ^ mrow[3][acc >> 24] ^ v;
	}
	if (c0 < c1 && y0 < y1) acc = gf2_mulmod(acc, r.tab[c1 - 1u]); else acc = 0u;
	acc = wave_xor32_dpp(acc);
	if (lane == 0u) wsum[wv] = y0 < y1 ? gf2_mulmod(acc, r.tab[r.quads + (r.h - y1)]) : 0u;
	__syncthreads();
	if (tid == 0u) {
		uint32_t x = 0;
		for (uint32_t k = 0; k < FEED_CRC_BS / 64u; ++k) x ^= wsum[k];
		atomicXor(r.raw + f, x);
	}
}

// The plane's CRC with ONE lookup per source byte, for rows of at most 64 groups (a lane has one group per row).  A grey dword takes
// 256 values and a lane starts every row from remainder 0, so its remainder over the n dwords of its group is XOR_i G[n - i][L_i],
// G[p][L] = R(grey(L)) x^(32 (p - 1)): sixteen independent lookups and an xor tree in the place of 64 dependent ones.  A thread
// builds column `tid` of G with the slice-by-4 step on a zero dword (G[p + 1] = G[p] x^32).  16 KB of LDS more.
__global__ void __launch_bounds__(FEED_CRC_BS) k_view_crc_gray1(FeedRun r) {
	__shared__ uint32_t tab[4][256], mrow[4][256], G[17][256], wsum[FEED_CRC_BS / 64u];
	const uint32_t f = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
	if (!r.res[f].map_open || r.res[f].status != SMHV_FRAME_OK) return;
	{
		uint32_t c = tid;
		for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? SMH_CRC_POLY : 0u);
		tab[0][tid] = c;
		const uint32_t xrow = r.tab[r.quads + 1u];
#pragma unroll
		for (uint32_t k = 0; k < 4u; ++k) mrow[k][tid] = gf2_mulmod(tid << (8u * k), xrow);
	}
	__syncthreads();
	{
		uint32_t c = tab[0][tid];
		for (int k = 1; k < 4; ++k) { c = (c >> 8) ^ tab[0][c & 255u]; tab[k][tid] = c; }
	}
	__syncthreads();
	{
		uint32_t c = view_gray(tid);
		G[0][tid] = 0u;                                                          // (p = 0: a dword that is not the message's)
		for (uint32_t p = 1; p <= 16u; ++p) {
			c = tab[3][c & 255u] ^ tab[2][(c >> 8) & 255u] ^ tab[1][(c >> 16) & 255u] ^ tab[0][c >> 24];
			G[p][tid] = c;
		}
	}
	__syncthreads();
	const bool live = lane < r.quads;                                            // (quads <= 64: the launcher's condition)
	const uint32_t y0 = min((blockIdx.x * (FEED_CRC_BS / 64u) + wv) * r.rows_per_wave, r.h), y1 = min(y0 + r.rows_per_wave, r.h);
	const uint8_t *frame = r.ui + (size_t)f * r.ui_stride + 16u * (live ? lane : 0u);
	const int32_t j0 = (int32_t)(16u * lane) - (int32_t)r.xoff;                   // message dword of the group's first pixel
	const int32_t pend = min(16, (int32_t)r.w - j0);                              // dwords from it to the group's last message dword
	uint32_t pos[16];                                                            // G's row of source byte i; 0 where the byte is not the message's
#pragma unroll
	for (int32_t i = 0; i < 16; ++i) pos[i] = (live && j0 + i >= 0 && i < pend) ? (uint32_t)(pend - i) : 0u;
	uint32_t acc = 0;
	for (uint32_t y = y0; y < y1; ++y) {
		const uint4 q = *(const uint4 *)(frame + (size_t)y * r.ui_pitch);
		const uint32_t d[4] = {q.x, q.y, q.z, q.w};
		uint32_t v = 0;
#pragma unroll
		for (uint32_t i = 0; i < 16u; ++i) v ^= G[pos[i]][(d[i >> 2] >> (8u * (i & 3u))) & 255u];
		acc = mrow[0][acc & 255u] ^ mrow[1][(acc >> 8) & 255u] ^ mrow[2][(acc >> 16) & 255u] ^ mrow[3][acc >> 24] ^ v;
	}
	if (live && y0 < y1) acc = gf2_mulmod(acc, r.tab[lane]); else acc = 0u;
	acc = wave_xor32_dpp(acc);
	if (lane == 0u) wsum[wv] = y0 < y1 ? gf2_mulmod(acc, r.tab[r.quads + (r.h - y1)]) : 0u;
	__syncthreads();
	if (tid == 0u) {
		uint32_t x = 0;
		for (uint32_t k = 0; k < FEED_CRC_BS / 64u; ++k) x ^= wsum[k];
		atomicXor(r.raw + f, x);
	}
}

// k_feed_maps for a view: destination driven as it is -- a lane owns four pixels of the payload, finds them in (row, column),
// makes their dwords from the source (a plane: four byte loads) and stores them as one aligned 16-byte store.
template <uint32_t SRC>
__global__ void __launch_bounds__(FEED_COPY_BS) k_feed_view_maps(FeedRun r) {
	const uint32_t n_maps = r.header->n_maps;
	if (!n_maps) return;
	const uint32_t dwords = r.w * r.h;
	const uint32_t groups = (dwords + 3u) >> 2, per_item = FEED_COPY_BS * FEED_COPY_GROUPS;
	const uint32_t items_per_map = (groups + per_item - 1u) / per_item;
	const uint64_t items = (uint64_t)n_maps * items_per_map;
	const uint32_t pitch_px = SRC == SMH_RND_SRC_GRAY ? (uint32_t)r.ui_pitch : (uint32_t)(r.ui_pitch >> 2);
	for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
		const uint32_t m = (uint32_t)(item / items_per_map), ib = (uint32_t)(item - (uint64_t)m * items_per_map);
		const FeedMap fm = r.maps[m];
		const uint8_t *src8 = r.ui + (size_t)fm.frame * r.ui_stride + r.xoff;
		const uint32_t *src32 = (const uint32_t *)(r.ui + (size_t)fm.frame * r.ui_stride) + r.xoff;
		uint8_t *dst = r.bytes + fm.dst;
		uint32_t d[FEED_COPY_GROUPS][4];
#pragma unroll
		for (uint32_t u = 0; u < FEED_COPY_GROUPS; ++u) {
			const uint32_t g = ib * per_item + u * FEED_COPY_BS + threadIdx.x;
			uint32_t q = min(4u * g, dwords - 1u), row = q / r.w, col = q - row * r.w;
#pragma unroll
			for (uint32_t k = 0; k < 4u; ++k) {
				const size_t at = (size_t)row * pitch_px + col;                              // (clamped to the view's last pixel: always inside the frame)
				d[u][k] = SRC == SMH_RND_SRC_GRAY ? (uint32_t)src8[at] : src32[at];
				if (q + 1u < dwords) { ++q; if (++col == r.w) { col = 0u; ++row; } }
			}
		}
#pragma unroll
		for (uint32_t u = 0; u < FEED_COPY_GROUPS; ++u) {
			const uint32_t g = ib * per_item + u * FEED_COPY_BS + threadIdx.x;
			if (g >= groups) continue;
			uint32_t o[4];
#pragma unroll
			for (uint32_t k = 0; k < 4u; ++k) o[k] = SRC == SMH_RND_SRC_GRAY ? view_gray(d[u][k]) : view_px<SRC>(d[u][k]);
			if (4u * g + 4u <= dwords) *(uint4 *)(dst + 16ull * g) = make_uint4(o[0], o[1], o[2], o[3]);
			else
				for (uint32_t k = 0; 4u * g + k < dwords; ++k) *(uint32_t *)(dst + 16ull * g + 4u * k) = o[k];
		}
	}
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
hipError_t launch_feed_view_tables(uint32_t *d_tab, uint32_t w, uint32_t h, uint32_t xoff, uint32_t quads, uint32_t ppg, hipStream_t s) {
	hipLaunchKernelGGL(k_feed_view_tables, dim3((quads + h + 255u) / 256u), dim3(256), 0, s, d_tab, w, h, xoff, quads, ppg);
	return hipGetLastError();
}

hipError_t launch_feed_tables(uint32_t *d_tab, uint32_t w, uint32_t h, uint32_t xoff, uint32_t quads, hipStream_t s) {
	hipLaunchKernelGGL(k_feed_tables, dim3((quads + h + 255u) / 256u), dim3(256), 0, s, d_tab, w, h, xoff, quads);
	return hipGetLastError();
}

// rows a wave of k_map_crc takes: as many as leave the launch some 2048 workgroups (eight per CU), at most 8
static std::atomic<uint32_t> g_feed_rows{0};            // smhv_debug_feed_rows
void feed_set_rows(uint32_t rows) { g_feed_rows.store(rows, std::memory_order_relaxed); }
uint32_t feed_rows_per_wave(uint32_t h, uint32_t n) {
	const uint32_t forced = g_feed_rows.load(std::memory_order_relaxed);
	if (forced) return forced;
	const uint64_t rows = (uint64_t)h * n;
	return (uint32_t)std::min<uint64_t>(8u, std::max<uint64_t>(1u, rows / (2048u * (FEED_CRC_BS / 64u))));
}

hipError_t launch_feed(const FeedRun &r, hipStream_t s) {
	hipError_t e = hipMemsetAsync(r.raw, 0, sizeof(uint32_t) * r.n, s);
	if (e != hipSuccess) return e;
	const uint32_t band = (FEED_CRC_BS / 64u) * r.rows_per_wave;
	hipLaunchKernelGGL(k_map_crc, dim3((r.h + band - 1u) / band, r.n), dim3(FEED_CRC_BS), 0, s, r);
	hipLaunchKernelGGL(k_feed_plan, dim3(1), dim3(FEED_PLAN_BS), 0, s, r);
	hipLaunchKernelGGL(k_feed_maps, dim3(2048), dim3(FEED_COPY_BS), 0, s, r);
	return hipGetLastError();
}

// a plane's CRC: 0 = the rule (one lookup per source byte where a row has at most 64 groups), 4 = four per message dword always
static std::atomic<uint32_t> g_feed_gray_form{0};       // smhv_debug_feed_gray_form
void feed_set_gray_form(uint32_t form) { g_feed_gray_form.store(form, std::memory_order_relaxed); }

hipError_t launch_feed_view(const FeedRun &r, uint32_t src_mode, hipStream_t s) {
	hipError_t e = hipMemsetAsync(r.raw, 0, sizeof(uint32_t) * r.n, s);
	if (e != hipSuccess) return e;
	const uint32_t band = (FEED_CRC_BS / 64u) * r.rows_per_wave;
	const dim3 grid((r.h + band - 1u) / band, r.n), bs(FEED_CRC_BS);
	switch (src_mode) {
	case SMH_RND_SRC_GRAY:
		if (r.quads <= 64u && g_feed_gray_form.load(std::memory_order_relaxed) != 4u) hipLaunchKernelGGL(k_view_crc_gray1, grid, bs, 0, s, r);
		else hipLaunchKernelGGL(k_view_crc<SMH_RND_SRC_GRAY>, grid, bs, 0, s, r);
		break;
	case SMH_RND_SRC_PREPROCESS: hipLaunchKernelGGL(k_view_crc<SMH_RND_SRC_PREPROCESS>, grid, bs, 0, s, r); break;
	case SMH_RND_SRC_CROPPED: hipLaunchKernelGGL(k_view_crc<SMH_RND_SRC_CROPPED>, grid, bs, 0, s, r); break;
	default: return hipErrorInvalidValue;
	}
	hipLaunchKernelGGL(k_feed_plan, dim3(1), dim3(FEED_PLAN_BS), 0, s, r);
	switch (src_mode) {
	case SMH_RND_SRC_GRAY: hipLaunchKernelGGL(k_feed_view_maps<SMH_RND_SRC_GRAY>, dim3(2048), dim3(FEED_COPY_BS), 0, s, r); break;
	case SMH_RND_SRC_PREPROCESS: hipLaunchKernelGGL(k_feed_view_maps<SMH_RND_SRC_PREPROCESS>, dim3(2048), dim3(FEED_COPY_BS), 0, s, r); break;
	default: hipLaunchKernelGGL(k_feed_view_maps<SMH_RND_SRC_CROPPED>, dim3(2048), dim3(FEED_COPY_BS), 0, s, r); break;
	}
	return hipGetLastError();
}

// The per-call path's view: one tight RGBA8 image.  `crc` describes it as rows of 1024 dwords behind a lead-in of zero dwords (leading
// zeros do not change the remainder), `r` as what it is -- the plan's and the copy's dimensions.
hipError_t launch_feed_image(const FeedRun &crc, const FeedRun &r, hipStream_t s) {
	hipError_t e = hipMemsetAsync(r.raw, 0, sizeof(uint32_t) * r.n, s);
	if (e != hipSuccess) return e;
	const uint32_t band = (FEED_CRC_BS / 64u) * crc.rows_per_wave;
	hipLaunchKernelGGL(k_map_crc, dim3((crc.h + band - 1u) / band, crc.n), dim3(FEED_CRC_BS), 0, s, crc);
	hipLaunchKernelGGL(k_feed_plan, dim3(1), dim3(FEED_PLAN_BS), 0, s, r);
	hipLaunchKernelGGL(k_feed_maps, dim3(2048), dim3(FEED_COPY_BS), 0, s, r);
	return hipGetLastError();
}

}  // namespace smh
