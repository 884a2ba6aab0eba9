// smh_lsd_seq.inc -- lsd::find_lines::<32> by ONE WAVE PER FRAME: the scan the frame-granular search service runs
// (smh_service.inc; included by smh_lsd.hip after smh_lsd_wave.inc, whose candidate set-up, window sampling and ray code it
// shares).
//
// k_lsd_tile spends a workgroup of 8-16 waves on a frame: candidates in a reorder buffer, units claimed with LDS atomics,
// a lock for retirement.  Measured (make wprof): those eight waves finish a frame only ~2.8x sooner than one wave working
// through the same units back to back would -- a candidate has 4 live units on average and the next candidate depends on
// its verdict, so most of a workgroup's wave-time is claiming, polling, lock waits and speculative casts that are thrown
// away.  What a batch's search takes from the chip is wave slots x time (DESIGN.md section 7), and one wave per frame takes a
// third of it (2.35 M wave-cycles per 1080p synthetic frame against 6.8 M).  The scan is the reference's own sequential loop,
// literally: next surviving white pixel in raster order -> get_centre -> the units the sector culling leaves, one after the
// other -> accept / reject.  No speculation, no atomics, no lock, nothing to retire out of order.  The price is latency -- the
// slowest synthetic frame takes 4 ms instead of 1 -- which is why it only became usable with frame-granular completion
// (round 4): as a batch launch it blocked its slot for as long as its slowest frame (200 k frames/s against 455 k).
// Results are the tile kernel's (and the oracle's) bit for bit: same candidate order, same rays, same arithmetic.
//
// The wave shares its CU with the HBM-bound streaming pass, whose loads keep the CU's vector-memory pipe backed up: a vector-
// memory access of this wave -- a global load, a spill reload -- waits ~2 us there (measured: set-up 4x, dispatch and verdict
// 3x slower than alone while the compiler kept 15 spill reloads in the candidate loop; tools/scratch_in_loops.py).  So inside
// the scan everything comes from LDS (mask tiles, window, lists, sector table, the 3600 ray directions) or through scalar
// loads, and the build checks that no scratch access sits in a loop.

// raster-ordered list of the non-zero mask words from (row0, skipping words with index < wi_min) on: -> entries stored;
// *wi_next = the first word that did not fit (WT when the scan reached the end of the window)
template <int MODE>
__device__ __forceinline__ uint32_t seq_build_list(const Win &m, WShared &ws, uint32_t *list, uint32_t *survw, uint32_t list_cap, uint32_t wy0, uint32_t wrows, uint32_t wwords, uint32_t wi_min,
                                                   uint32_t WT, uint32_t *wi_next) {
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t o = 0, next = WT;
	// one set of lanes' words into the list (raster order = lane order); -> false when the list is full
	auto append = [&](uint32_t w, uint32_t wi) {
		const unsigned long long nz = __ballot(w != 0u);
		if (!nz) return;
		const uint32_t pos = o + (uint32_t)__popcll(nz & ((1ull << lane) - 1ull));
		if (w != 0u && pos < list_cap) { list[pos] = wi; survw[pos] = w; ws.stag[pos] = 0; }
		const uint32_t cnt = (uint32_t)__popcll(nz);
		if (o + cnt > list_cap) {                                      // the (list_cap - o)-th set lane holds the first word that did not fit
			unsigned long long rest = nz;
			for (uint32_t k = o; k < list_cap; ++k) rest &= rest - 1ull;
			next = (uint32_t)__builtin_amdgcn_readlane((int)wi, (int)__builtin_ctzll(rest));
			o = list_cap;
		} else o += cnt;
	};
	if constexpr (MODE == LSD_MODE_TILE || MODE == LSD_MODE_TILEC) {
		// (the tile of word column c in tile row ty: through the 16-bit table, or the compact index of LSD_MODE_TILEC)
		auto tile_at = [&](uint32_t ty, uint32_t c) -> uint32_t {
			if constexpr (MODE == LSD_MODE_TILEC) return tilec_number(m, (int)c, (int)ty);
			else return (uint32_t)m.t_idx[__mul24((int)ty, (int)m.t_pitch) + (int)c];
		};
		// Tile row by tile row (8 mask rows share their index entries: one look decides for all eight -- most tile rows of a
		// map hold no marker pixel -- instead of one look per mask row), and two mask rows per step where a row's words fit half
		// a wave (up to 1024 px of ROI width: 1080p).  The scan was 822 dependent LDS round trips per 1080p frame, a tenth of a
		// frame's search time in the loaded pipeline.
		const bool two = wwords <= 32u;
		const uint32_t sub = two ? lane >> 5 : 0u, cl = two ? lane & 31u : lane;
		const uint32_t y_end = wy0 + wrows;
		if (wwords <= 64u) {
			for (uint32_t y = wy0 + wi_min / wwords; y < y_end && next == WT;) {
				const uint32_t y_tile_end = min((y | 7u) + 1u, y_end);
				const uint32_t t = cl < wwords ? tile_at(y >> 3, cl) : 0u;
				if (__any(t != 0u)) {
					for (uint32_t yy = y; yy < y_tile_end && next == WT; yy += two ? 2u : 1u) {
						const uint32_t yr = yy + sub;
						const uint32_t wi = (yr - wy0) * wwords + cl;
						uint32_t w = (t && yr < y_tile_end) ? (uint32_t)m.t_tiles[(t << 3) + (yr & 7u)] : 0u;
						if (wi < wi_min) w = 0u;
						append(w, wi);
					}
				}
				y = y_tile_end;
			}
		} else {                                                      // (rows wider than a wave: 8K frames; row by row)
			for (uint32_t y = wy0 + wi_min / wwords; y < y_end && next == WT; ++y) {
				for (uint32_t c0 = 0; c0 < wwords && next == WT; c0 += 64u) {
					const uint32_t c = c0 + lane;
					const uint32_t t = c < wwords ? tile_at(y >> 3, c) : 0u;
					if (!__any(t != 0u)) continue;
					const uint32_t wi = (y - wy0) * wwords + c;
					uint32_t w = t ? (uint32_t)m.t_tiles[(t << 3) + (y & 7u)] : 0u;
					if (wi < wi_min) w = 0u;
					append(w, wi);
				}
			}
		}
	} else {
		for (uint32_t r = wi_min / wwords; r < wrows && next == WT; ++r) {
			for (uint32_t c0 = 0; c0 < wwords && next == WT; c0 += 64u) {
				const uint32_t c = c0 + lane;
				const uint32_t wi = r * wwords + c;
				uint32_t w = c < wwords ? m.p[r * wwords + c] : 0u;     // LSD_MODE_GLOBAL: the domain is the window of the global mask (frame_setup)
				if (wi < wi_min) w = 0u;
				append(w, wi);
			}
		}
	}
	*wi_next = next;
	return o;
}

// ---- the help desk: waves of the same workgroup casting a heavy frame's upcoming candidates --------------------------------
// The scan is sequential only through the accepted lines: whether a pixel is VISITED depends on the lines accepted before it,
// what casting it yields does not (a pure function of mask and pixel).  Most visited candidates are rejected (157 rounds for
// 7 lines on the slowest synthetic frame, 372 for 24 on the heaviest screenshot), so the pixels the scan will visit next are,
// with few exceptions, the next survivors in raster order as the list stands.  A frame that has been at work for
// SEQ_HELP_AFTER rounds posts those pixels on a desk in its own LDS block; a wave of the same workgroup that has finished its
// own frame takes one, casts it on the OWNER's mask tiles (its own candidate window), and leaves the result there; the owner,
// arriving at a pixel, takes the result if there is one (waits if it is being cast, takes an untouched post back and casts it
// itself).  A post whose pixel a newly accepted line removed is simply never asked for.  The owner visits exactly the pixels
// of the sequential scan in exactly its order: lines, rounds and sample counts are the reference's, whoever cast what.
#define SEQ_HELP_SLOTS 4u               // desk entries = candidates posted ahead (WShared::rob[0 .. SEQ_HELP_SLOTS))
#define SEQ_MAX_HELPERS 3u
#ifndef SEQ_RAY_GROUP
#define SEQ_RAY_GROUP 16                // samples of a ray's first batches whose window reads are in flight together (ray_batch) ...
#endif
#ifndef SEQ_RAY_GROUP_C
#define SEQ_RAY_GROUP_C 32              // ... a whole batch behind the compact index (LSD_MODE_TILEC: the service kernel with the 168-register budget, smh_service.inc)
#endif
#ifndef SEQ_HELP_AFTER
#define SEQ_HELP_AFTER 8u               // rounds a frame works alone before it asks (a mean synthetic frame has 53)
#endif
enum { H_FREE = W_FREE, H_POSTED = W_SETUP, H_TAKEN = W_CASTING, H_DONE = W_DONE, H_RPOSTED = 5, H_RZOMBIE = 6 };

// ---- the desk across workgroups (smh_kernels.h, SvcRemote) -----------------------------------------------------------------
// rob[0 .. SEQ_HELP_SLOTS) is the workgroup's desk: helpers read and write those entries in LDS.  rob[SEQ_HELP_SLOTS ..
// SEQ_DESK_ENTRIES) is the owner's BOOK of the posts it has out in global memory (SvcRemote::ring, entry e of the ring = book
// entry SEQ_HELP_SLOTS + e): pixel, the post's number k (in `lines_seen`) and
//   H_RPOSTED  posted; nobody of this wave knows more
//   H_DONE     the result has been fetched into the book (remote_harvest)
//   H_RZOMBIE  the scan no longer wants it but a helper had already taken it: the entry is free again when that result is in
// Only the owner wave touches the book.  Taking a post -- a helper to cast it, the owner to take it back or to cancel it -- is
// an atomic max on the ring entry's `claim` word with the post's number: whoever raises it from below k has it.
#define SEQ_DESK_ENTRIES (SEQ_HELP_SLOTS + SVC_REMOTE_RING)
#ifdef SMH_LSD_WDEBUG
#define RDBG(i, v) do { if ((threadIdx.x & 63u) == 0) ws.rdbg[i] += (v); } while (0)
#else
#define RDBG(i, v)
#endif
#define SEQ_REMOTE_MIN_LEFT 12u         // list entries a frame must still have in front of it to ask the other workgroups
static_assert(SEQ_DESK_ENTRIES <= W_ROB, "the book of remote posts fits the reorder buffer's entries");
__device__ __forceinline__ SvcRemote *rem_of(const WShared &ws) {
	const unsigned long long v = ws.rem_r;
	return (SvcRemote *)(uintptr_t)(((unsigned long long)uniform_u32((uint32_t)(v >> 32)) << 32) | uniform_u32((uint32_t)v));
}
__device__ __forceinline__ void wave_lds_sync() {
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// 16-byte granules of the result exchange: write-through store / L2-bypassing load (`sc0 sc1`), one instruction each
typedef uint32_t rem_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void g_st128(uint32_t *p, rem_u32x4 v) { asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" : : "v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ void g_ld128x2(const uint32_t *p, rem_u32x4 &a, rem_u32x4 &b) {
	asm volatile("global_load_dwordx4 %0, %2, off sc0 sc1\n\tglobal_load_dwordx4 %1, %2, off offset:16 sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(a), "=&v"(b) : "v"(p) : "memory");
}
// owner: the results that have come back -> the book, in ONE round trip (both halves of every entry that is out; a half is valid
// when it carries the post's number).  -> helpers attached to the request (lane SVC_REMOTE_RING reads the state word alongside)
__device__ __forceinline__ uint32_t remote_harvest(WShared &ws) {
	const uint32_t lane = opaque_lane();
	RDBG(4, 1ull);
	SvcRemote *r = rem_of(ws);
	const bool mine = lane < SVC_REMOTE_RING;
	WSlot &sl = ws.rob[SEQ_HELP_SLOTS + (mine ? lane : 0u)];
	const uint32_t st = mine ? sl.state : (uint32_t)H_FREE, k = sl.lines_seen;
	const bool out = st == (uint32_t)H_RPOSTED || st == (uint32_t)H_RZOMBIE;
	rem_u32x4 a = {0u, 0u, 0u, 0u}, b = {0u, 0u, 0u, 0u};
	unsigned long long stw = 0ull;
	if (out) g_ld128x2(r->ring[lane].res_a, a, b);
	else if (lane == SVC_REMOTE_RING) stw = g_ld64(&r->state);
	if (out && a.x == k && b.x == k) {
		if (st == (uint32_t)H_RZOMBIE) sl.state = H_FREE;
		else {
			sl.best = ((unsigned long long)a.z << 32) | a.w; sl.steps = a.y;
			sl.ex = __uint_as_float(b.y); sl.ey = __uint_as_float(b.z);
			sl.ptx = 0.5f * (float)(b.w & 0xFFFFu); sl.pty = 0.5f * (float)(b.w >> 16);
			sl.state = H_DONE;
		}
	}
	wave_lds_sync();
	return (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)stw, (int)SVC_REMOTE_RING) & 0x7FFFFFFFu;
}
// owner: helpers of other workgroups attached to the open request
__device__ __forceinline__ uint32_t remote_helpers(WShared &ws) {
	const unsigned long long st = g_ld64(&rem_of(ws)->state);
	return uniform_u32((uint32_t)st & 0x7FFFFFFFu);
}
// owner, at the end of its frame: the request closes (helpers leave when they next look; what they still write goes to ring
// entries nobody reads before the next request has reset them, and that request waits until they have all gone)
__device__ __forceinline__ void remote_close(WShared &ws) {
	if ((threadIdx.x & 63u) == 0u) {
		__hip_atomic_fetch_and(&rem_of(ws)->state, ~SVC_REMOTE_OPEN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		ws.rem_open = 0u;
	}
	wave_lds_sync();
}
// owner: `tickets` tickets for the wave's open request into the service's help ring (lane 0's work; every lane gets the answer).
// The tickets are counted first -- a popper that is quicker than the entries waits for its entry -- and not at all while the ring
// is half full (tickets nobody has time for: the chip is busy with frames).
__device__ __forceinline__ bool remote_issue_tickets(WShared &ws, SvcCtl *ctl, uint32_t gen, uint32_t tickets) {
	uint32_t ok = 0;
	if ((threadIdx.x & 63u) == 0u && tickets) {
		if (__hip_atomic_fetch_add(&ctl->help_avail, (int32_t)tickets, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + (int32_t)tickets <= (int32_t)(SVC_HELP_RING / 2u)) {
			const uint32_t base = __hip_atomic_fetch_add(&ctl->help_reserve, tickets, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			for (uint32_t t = 0; t < tickets; ++t) {
				const uint32_t tk = base + t;
				g_st64(&ctl->help_ring[tk & (SVC_HELP_RING - 1u)], ((unsigned long long)(tk / SVC_HELP_RING + 1u) << 32) | ((gen & 0xFFFFu) << 16) | (ws.rem_owner & 0xFFFFu));
			}
			ok = 1u;
		} else __hip_atomic_fetch_sub(&ctl->help_avail, (int32_t)tickets, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	return uniform_u32(ok) != 0u;
}
__device__ __forceinline__ SvcCtl *rem_ctl_of(const WShared &ws) {
	return (SvcCtl *)(uintptr_t)(((unsigned long long)uniform_u32((uint32_t)(ws.rem_ctl >> 32)) << 32) | uniform_u32((uint32_t)ws.rem_ctl));
}
// owner: ask the other workgroups.  The frame's tile store (the words a helper needs: the used tiles and the index) goes to the
// wave's block of SvcParams::remote_store, the ring is reset, the request opens and `rem_tickets` tickets go into the help
// ring.  Not now (-> false) while a helper of an earlier request of this wave has not left, or while the help ring is busy.
// (A real call: once per frame at most, and its copy loops must not cost the scan registers.)
template <bool COMPACT>
__device__ __attribute__((noinline)) bool remote_open(uint32_t ws_off, uint32_t store_off, uint32_t idx_words) {
	WShared &ws = *(WShared *)(LdsWord *)(uintptr_t)uniform_u32(ws_off);
	const uint32_t lane = threadIdx.x & 63u;
	SvcRemote *r = rem_of(ws);
	SvcCtl *ctl = rem_ctl_of(ws);
	uint32_t *dump = (uint32_t *)(uintptr_t)(((unsigned long long)uniform_u32((uint32_t)(ws.rem_store >> 32)) << 32) | uniform_u32((uint32_t)ws.rem_store));
	const uint32_t tickets = uniform_u32(ws.rem_tickets), tile_cap = uniform_u32(ws.rem_cap), ntiles = min(uniform_u32(ws.ntiles), tile_cap);
	const unsigned long long st = g_ld64(&r->state);
	const uint32_t st_lo = uniform_u32((uint32_t)st), st_hi = uniform_u32((uint32_t)(st >> 32));
	if (st_lo != 0u) return false;                                 // open (never: this wave closes what it opens) or a helper still attached
	if ((int32_t)uniform_u32((uint32_t)__hip_atomic_load(&ctl->help_avail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) > (int32_t)(SVC_HELP_RING / 4u)) return false;   // tickets nobody has time for
	const uint4 *src = (const uint4 *)(LdsWord *)(uintptr_t)uniform_u32(store_off);
	uint4 *dst = (uint4 *)dump;
	for (uint32_t i = lane; i < (ntiles + 1u) * 2u; i += 64u) dst[i] = src[i];
	const uint32_t q0 = (tile_cap + 1u) * 2u, nq = (idx_words + 3u) / 4u;
	for (uint32_t i = lane; i < nq; i += 64u) dst[q0 + i] = src[q0 + i];
	if (lane < SVC_REMOTE_RING) {
		const rem_u32x4 z = {0u, 0u, 0u, 0u};
		g_st64(&r->ring[lane].post, 0ull); g_st64(&r->ring[lane].claim, 0ull); g_st128(r->ring[lane].res_a, z); g_st128(r->ring[lane].res_b, z);
	}
	if (lane == 0) g_st64(&r->info, (unsigned long long)ntiles);
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	uint32_t gen = st_hi + 1u;
	if ((gen & 0xFFFFu) == 0u) ++gen;                              // (a ticket names the request by 16 bits of its number: never 0)
	if (lane == 0) {
		g_st64(&r->state, ((unsigned long long)gen << 32) | SVC_REMOTE_OPEN);
		__hip_atomic_fetch_add(&ctl->stat_requests, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		ws.rem_open = 1u; ws.rem_gen = gen; ws.rem_k = 0u; ws.rem_nr = 0u;
	}
	wave_lds_sync();
	(void)remote_issue_tickets(ws, ctl, gen, tickets);          // (none now: the owner asks again as it goes)
	return true;
}

// The mask of a frame as its tile store in LDS describes it (what frame_setup_tile returns in FrameView::m)
__device__ __forceinline__ void tile_win(Win &m, uint32_t rw, uint32_t rh, uint32_t *smem, uint32_t tile_cap) {
	const uint32_t TWP = tile_idx_pitch(rw);
	m.w = rw; m.h = rh; m.wf = (float)rw; m.hf = (float)rh;
	m.p = smem; m.pitch4 = 0u; m.y_lo = 0; m.xbias = 0; m.rows_hi = 0u; m.cols_hi = 0u;
	m.rows0 = nullptr; m.ylo_f = 0.0f; m.yhi_f = 0.0f;
	m.c_p = (const LdsWord *)smem; m.c_y0 = 0u; m.c_rows = 0u; m.c_pitch4 = 0u;
	m.t_idx = (const LdsU16 *)(smem + (tile_cap + 1u) * 8u) + TWP + 2u; m.t_tiles = (const LdsWord *)smem; m.t_pitch = TWP; m.tiled = true;
	m.tc_rows = nullptr; m.tc_groups = 0u; m.compact = false;
	m.w2 = nullptr;
}

// ... and behind the compact index (what frame_setup_tilec returns)
__device__ __forceinline__ void tilec_win(Win &m, uint32_t rw, uint32_t rh, uint32_t *smem, uint32_t tile_cap) {
	tile_win(m, rw, rh, smem, tile_cap);
	const uint32_t G = tilec_groups(rw);
	m.t_idx = nullptr;
	m.tc_rows = (const LdsWord *)(smem + (tile_cap + 1u) * 8u + G * 4u); m.tc_groups = G; m.compact = true;
}

// The service's candidate window.  In k_lsd_service a wave casts one candidate after the other in ONE window block, and the block
// keeps its window from candidate to candidate (WinTag, smh_lsd_wave.inc): a fill happens only when the next candidate reads
// outside it, and covers SVC_WIN_EXTRA rows BELOW its candidate's needed region, so that the scan's next rows find their window
// there too (6 words of LDS per row and wave; svc_waves_for counts them).  k_lsd_service_c (the compact index, above 1080p) fills
// 135 rows for every candidate as before: measured, reuse buys nothing there (DESIGN.md section 5).
// -DSMH_NO_WINDOW_REUSE: the same in k_lsd_service -- the code before the tag (the A/B switch).
#ifndef SVC_WIN_EXTRA
#define SVC_WIN_EXTRA 24u               // measured among 0, 8, 16, 24 on the headline (DESIGN.md section 5, profiles/window_reuse_sweep.json); the geometry at 1080p is the same
#endif
#ifdef SMH_NO_WINDOW_REUSE
#define SVC_WIN_REUSE(compact) false
#else
#define SVC_WIN_REUSE(compact) (!(compact))
#endif
#define SVC_WIN_ROWS(compact) (SVC_WIN_REUSE(compact) ? W_WIN_ROWS + SVC_WIN_EXTRA : W_WIN_ROWS)
#define SVC_WIN_STRIDE(compact) (SVC_WIN_ROWS(compact) * LSD_W2_PITCH + 2u)   // words per service window block (as W_WIN_STRIDE)
// The service's own sampler of a ray's first batches (ray_batch<.., LEAN>, smh_lsd.hip): k_lsd_service alone; k_lsd_service_c keeps
// the 32-sample groups of ray_batch as they were.  -DSMH_NO_LEAN_SAMPLER: the sampler before it (the A/B switch).
#ifdef SMH_NO_LEAN_SAMPLER
#define SVC_LEAN_SAMPLER(compact) false
#else
#define SVC_LEAN_SAMPLER(compact) (!(compact))
#endif

// One candidate from its pixel to its longest ray, by one wave: window + get_centre + sector culling (cand_setup), then its
// live 64-ray units one after the other (the next unit's directions fetched while this one is cast).
// -> start point; wkey = len^2 bits << 32 | ray index of the longest exactly evaluated ray (0: none could make a line), its end
// point; mask samples taken (sum over the wave)
// REUSE: `wwin` holds the window `tag` places (W_WIN_ROWS + SVC_WIN_EXTRA rows) and is filled only when it does not serve; else: filled for this candidate
// LEAN: the rays' first batches through the service's own sampler (ray_batch, smh_lsd.hip)
template <int MODE, bool REUSE = false, bool LEAN = false>
__device__ __forceinline__ void seq_cast_candidate(const Win &m, uint32_t *wwin, WinTag *tag, const uint32_t *cull_tab, uint32_t cull, const RayDir *dirs, const float *ray_off, float max_gap,
                                                   uint32_t px, uint32_t py, float &xs, float &ys, unsigned long long &wkey, float &ex0, float &ey0, uint32_t &steps_sum
#ifdef SMH_LSD_WDEBUG
                                                   , unsigned long long *sprof, unsigned long long &slast, unsigned long long *uprof, uint32_t &n_units
#endif
                                                   ) {
	const uint32_t lane = opaque_lane();
	unsigned long long live;
#ifdef SMH_LSD_WDEBUG
	cand_setup<MODE == LSD_MODE_TILEC, (REUSE ? W_WIN_ROWS + SVC_WIN_EXTRA : W_WIN_ROWS), REUSE>(m, wwin, cull_tab, cull, px, py, xs, ys, live, tag, uprof);
	{ const unsigned long long _n = __builtin_amdgcn_s_memtime(); sprof[2] += _n - slast; slast = _n; }
#else
	cand_setup<MODE == LSD_MODE_TILEC, (REUSE ? W_WIN_ROWS + SVC_WIN_EXTRA : W_WIN_ROWS), REUSE>(m, wwin, cull_tab, cull, px, py, xs, ys, live, tag);
#endif
	unsigned long long bkey = 0ull;
	float bxe = xs, bye = ys;
	uint32_t st = 0;
	auto unit_dirs_lds = [&](uint32_t u) -> RayDir { return dirs[min(u * 64u + lane, (uint32_t)SMH_LSD_RAYS - 1u)]; };
	RayDir dn = unit_dirs_lds(live ? (uint32_t)__builtin_ctzll(live) : 0u);
	for (unsigned long long todo = live; todo; todo &= todo - 1ull) {
		const uint32_t u = (uint32_t)__builtin_ctzll(todo);
		const RayDir d = dn;
		const unsigned long long rest = todo & (todo - 1ull);
		if (rest) dn = unit_dirs_lds((uint32_t)__builtin_ctzll(rest));
		unsigned long long key;
		float xe, ye;
#ifdef SMH_LSD_WDEBUG
		unit_rays<MODE, (MODE == LSD_MODE_TILEC ? SEQ_RAY_GROUP_C : SEQ_RAY_GROUP), REUSE, LEAN>(m, wwin, ray_off, px, py, xs, ys, u, d, max_gap, key, xe, ye, st, uprof, tag);
		++n_units;
#else
		unit_rays<MODE, (MODE == LSD_MODE_TILEC ? SEQ_RAY_GROUP_C : SEQ_RAY_GROUP), REUSE, LEAN>(m, wwin, ray_off, px, py, xs, ys, u, d, max_gap, key, xe, ye, st, tag);
#endif
		if (key > bkey) { bkey = key; bxe = xe; bye = ye; }
	}
	steps_sum = wave_sum32_dpp(st);
	// the longest ray, ties -> highest angle (vision-cpu/src/lib.rs:440-446): max of the unique keys
	wkey = 0ull; ex0 = xs; ey0 = ys;
	if (__any(bkey != 0ull)) {
		const uint32_t hi = (uint32_t)(bkey >> 32), lo = (uint32_t)bkey;
		const uint32_t mhi = wave_max32_dpp(hi);
		const uint32_t mlo = wave_max32_dpp(hi == mhi ? lo : 0u);
		wkey = ((unsigned long long)mhi << 32) | mlo;
		if (wkey != 0ull) {
			const uint32_t src = (uint32_t)__builtin_ctzll(__ballot(bkey == wkey));
			ex0 = bcast_f(bxe, src); ey0 = bcast_f(bye, src);
		}
	}
#ifdef SMH_LSD_WDEBUG
	{ const unsigned long long _n = __builtin_amdgcn_s_memtime(); sprof[3] += _n - slast; slast = _n; }
#endif
}

// owner: is there a result (or a cast in progress) for the pixel the scan has arrived at?  -> true with the result
__device__ __forceinline__ bool desk_take(WShared &ws, uint32_t px, uint32_t py, float &xs, float &ys, unsigned long long &wkey, float &ex0, float &ey0, uint32_t &steps_sum) {
	const uint32_t lane = opaque_lane();
	bool match = false;
	if (lane < SEQ_DESK_ENTRIES) {
		const uint32_t st = W_LD_ACQ(&ws.rob[lane].state);
		match = st != (uint32_t)H_FREE && st != (uint32_t)H_RZOMBIE && ws.rob[lane].px == px && ws.rob[lane].py == py;
	}
	const unsigned long long hit = __ballot(match);
	if (!hit) return false;
	const uint32_t e = (uint32_t)__builtin_ctzll(hit);
	WSlot &sl = ws.rob[e];
	if (e >= SEQ_HELP_SLOTS) {
		// a post to the other workgroups: what has come back, first
		if (uniform_u32(sl.state) == (uint32_t)H_RPOSTED) remote_harvest(ws);
		WDBG(0, 1u);                                                 // (diagnostic build: arrivals at a pixel posted to other workgroups)
		if (uniform_u32(sl.state) == (uint32_t)H_RPOSTED) {
			// not back yet: nobody has started on it -> the owner takes it back and casts it itself; being cast -> less left to wait for than to redo
			const uint32_t k = uniform_u32(sl.lines_seen);
			uint32_t old = 0;
			if (lane == 0) old = (uint32_t)__hip_atomic_fetch_max(&rem_of(ws)->ring[e - SEQ_HELP_SLOTS].claim, (unsigned long long)k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			if (uniform_u32(old) < k) {
				if (lane == 0) sl.state = H_FREE;
				wave_lds_sync();
				WDBG(1, 1u);                                             // ... taken back
				return false;
			}
			WDBG(2, 1u);                                                 // ... waited for
#ifdef SMH_LSD_WDEBUG
			const unsigned long long t_w = __builtin_amdgcn_s_memtime();
#endif
			while (uniform_u32(sl.state) != (uint32_t)H_DONE) { __builtin_amdgcn_s_sleep(16); remote_harvest(ws); }
#ifdef SMH_LSD_WDEBUG
			if (lane == 0) ws.prof[0] += __builtin_amdgcn_s_memtime() - t_w;
#endif
		}
		xs = sl.ptx; ys = sl.pty; wkey = sl.best; ex0 = sl.ex; ey0 = sl.ey; steps_sum = sl.steps;
		__builtin_amdgcn_wave_barrier();
		if (lane == 0) sl.state = H_FREE;
		wave_lds_sync();
		return true;
	}
	if (uniform_u32(W_LD_ACQ(&sl.state)) == (uint32_t)H_POSTED) {   // nobody has started on it: take it back
		uint32_t ok = 0;
		if (lane == 0) { uint32_t expect = H_POSTED; ok = __hip_atomic_compare_exchange_strong(&sl.state, &expect, (uint32_t)H_FREE, __ATOMIC_ACQ_REL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) ? 1u : 0u; }
		if (uniform_u32(ok)) return false;
	}
	while (uniform_u32(W_LD_ACQ(&sl.state)) != (uint32_t)H_DONE) __builtin_amdgcn_s_sleep(2);   // being cast: less left to wait for than to redo
	xs = sl.ptx; ys = sl.pty; wkey = sl.best; ex0 = sl.ex; ey0 = sl.ey; steps_sum = sl.steps;
	__builtin_amdgcn_wave_barrier();
	if (lane == 0) W_ST_REL(&sl.state, (uint32_t)H_FREE);
	return true;
}

// One list entry as the dispatcher sees it: its survivor word brought up to date with the accepted lines (wave_dispatch's own
// rule, shared with the look-ahead below) -> w, and the coordinates of its bit 0
__device__ __forceinline__ uint32_t disp_entry(WShared &ws, const uint32_t *list, uint32_t *survw, uint32_t e, uint32_t first, uint32_t end, uint32_t n_lines, uint32_t wy0, uint32_t wwords,
                                               int xorg, float &fpx0, float &fpy) {
	uint32_t w = 0;
	fpx0 = 0.0f; fpy = 0.0f;
	if (e < end && e >= first) {
		w = survw[e];
		const uint32_t wi = list[e], r = wi / wwords, c = wi - r * wwords;
		fpy = (float)(wy0 + r); fpx0 = (float)(xorg + (int)(c * 32u));
		const uint32_t tag = ws.stag[e];
		if (w && tag < n_lines) {
			for (uint32_t l = tag; l < n_lines && w; ++l) {
				ProxLine L;
				L.x0 = ws.lines[l][0]; L.y0 = ws.lines[l][1]; L.x1 = ws.lines[l][2]; L.y1 = ws.lines[l][3];
				L.a = ws.prox_a[l]; L.dxl = ws.prox_d[l][0]; L.dyl = ws.prox_d[l][1];
				L.degenerate = L.dxl == 0.0 && L.dyl == 0.0;
				w = prox_filter_word(w, fpx0, fpy, L);
			}
			survw[e] = w;
			ws.stag[e] = (unsigned char)n_lines;
		}
	}
	return w;
}

// owner, after a verdict: the desk follows the scan.  Posts whose pixel is no longer among the next survivors are dropped,
// and of the next 1 + cap_local + cap_remote survivors all but the FIRST are posted if they are not on the desk yet: the nearest
// on the workgroup's desk (oldest first: `lines_seen` carries a running number, a helper takes the lowest), the ones further
// along in the ring of the other workgroups' helpers (whose answers take microseconds to travel).  The first is the owner's own
// next candidate: it casts that one itself while the helpers cast the ones behind it -- posted, the owner would arrive at it a
// moment later, find it taken, and wait.
// -> (cur_e, cur_bit): the list position of the last survivor looked at (desk_post_more goes on from there)
__device__ __forceinline__ void desk_post_remote(WShared &ws, uint32_t slot, uint32_t qx, uint32_t qy, uint32_t &st, uint32_t &spx, uint32_t &spy) {
	const uint32_t k = uniform_u32(ws.rem_k) + 1u;
	if (opaque_lane() == slot) {
		ws.rob[slot].px = qx; ws.rob[slot].py = qy; ws.rob[slot].lines_seen = k; ws.rob[slot].state = H_RPOSTED;
		ws.rem_k = k;
		g_st64(&rem_of(ws)->ring[slot - SEQ_HELP_SLOTS].post, ((unsigned long long)k << 32) | ((qy & 0xFFFFu) << 16) | (qx & 0xFFFFu));
		st = H_RPOSTED; spx = qx; spy = qy;
	}
	RDBG(0, 1ull);
	wave_lds_sync();
}
__device__ __forceinline__ void desk_refresh(WShared &ws, const uint32_t *list, uint32_t *survw, uint32_t wy0, uint32_t wwords, int xorg, uint32_t cap_local, uint32_t cap_remote, uint32_t &post_seq,
                                             uint32_t &cur_e, int &cur_bit, uint32_t &ahead) {
	const uint32_t lane = opaque_lane();
	const uint32_t n_lines = W_LD(&ws.n_lines), end = ws.disp_end, first = W_LD(&ws.disp_e);
	const uint32_t want = 1u + cap_local + cap_remote;           // <= SEQ_DESK_ENTRIES + 1
	cur_e = end; cur_bit = -1;                                   // (fewer than `want` survivors left: nothing beyond them)
	// ---- the next survivors in raster order, without consuming them: lane k holds the k-th ----
	uint32_t mpx = 0xFFFFFFFFu, mpy = 0xFFFFFFFFu, np = 0;
	for (uint32_t e0 = first & ~63u; e0 < end && np < want; e0 += 64u) {
		float fpx0, fpy;
		const uint32_t w = disp_entry(ws, list, survw, e0 + lane, first, end, n_lines, wy0, wwords, xorg, fpx0, fpy);
		unsigned long long any = __ballot(w != 0u);
		while (any && np < want) {
			const uint32_t src = (uint32_t)__builtin_ctzll(any);
			any &= any - 1ull;
			uint32_t ww = (uint32_t)__builtin_amdgcn_readlane((int)w, (int)src);
			const int bx = (int)bcast_f(fpx0, src);
			const uint32_t by = (uint32_t)bcast_f(fpy, src);
			while (ww && np < want) {
				const uint32_t bit = (uint32_t)__builtin_ctz(ww);
				ww &= ww - 1u;
				if (lane == np) { mpx = (uint32_t)(bx + (int)bit); mpy = by; }
				++np;
				if (np == want) { cur_e = e0 + src; cur_bit = (int)bit; }
			}
		}
	}
	ahead = np;                                                  // survivors looked at that the scan has not visited yet (its own next first)
	// ---- drop what the scan will not ask for (lane e looks after entry e) ----
	uint32_t st = H_FREE, spx = 0, spy = 0, sk = 0;
	if (lane < SEQ_DESK_ENTRIES) { st = W_LD_ACQ(&ws.rob[lane].state); spx = ws.rob[lane].px; spy = ws.rob[lane].py; sk = ws.rob[lane].lines_seen; }
	bool listed = false;
	for (uint32_t k = 0; k < np; ++k) {
		const uint32_t qx = (uint32_t)__builtin_amdgcn_readlane((int)mpx, (int)k), qy = (uint32_t)__builtin_amdgcn_readlane((int)mpy, (int)k);
		listed = listed || (spx == qx && spy == qy);
	}
	if (lane < SEQ_HELP_SLOTS && !listed) {
		if (st == (uint32_t)H_DONE) { W_ST(&ws.rob[lane].state, (uint32_t)H_FREE); st = H_FREE; }
		else if (st == (uint32_t)H_POSTED) {
			uint32_t expect = H_POSTED;
			if (__hip_atomic_compare_exchange_strong(&ws.rob[lane].state, &expect, (uint32_t)H_FREE, __ATOMIC_ACQ_REL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) st = H_FREE;
			else st = H_TAKEN;                              // a helper got there first: its result is dropped by a later refresh
		}
	}
	if (lane >= SEQ_HELP_SLOTS && lane < SEQ_DESK_ENTRIES && !listed) {
		if (st == (uint32_t)H_DONE) { ws.rob[lane].state = H_FREE; st = H_FREE; }
		else if (st == (uint32_t)H_RPOSTED) {               // cancel: free at once unless a helper has it (then: when its result is in)
			const unsigned long long old = __hip_atomic_fetch_max(&rem_of(ws)->ring[lane - SEQ_HELP_SLOTS].claim, (unsigned long long)sk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			st = (uint32_t)old < sk ? (uint32_t)H_FREE : (uint32_t)H_RZOMBIE;
			ws.rob[lane].state = st;
#ifdef SMH_LSD_WDEBUG
			atomicAdd(&ws.rdbg[st == (uint32_t)H_FREE ? 1 : 2], 1ull);
#endif
		}
	}
	wave_lds_sync();
	// ---- post the survivors that are not on the desk ----
	for (uint32_t k = 1; k < np; ++k) {
		const uint32_t qx = (uint32_t)__builtin_amdgcn_readlane((int)mpx, (int)k), qy = (uint32_t)__builtin_amdgcn_readlane((int)mpy, (int)k);
		const bool live = lane < SEQ_DESK_ENTRIES && st != (uint32_t)H_FREE && st != (uint32_t)H_RZOMBIE;
		if (__ballot(live && spx == qx && spy == qy) != 0ull) continue;
		const unsigned long long free_l = __ballot(lane < SEQ_HELP_SLOTS && st == (uint32_t)H_FREE);
		const unsigned long long free_r = __ballot(lane >= SEQ_HELP_SLOTS && lane < SEQ_DESK_ENTRIES && st == (uint32_t)H_FREE);
		const uint32_t busy_l = SEQ_HELP_SLOTS - (uint32_t)__popcll(free_l);
		const uint32_t busy_r = (uint32_t)__popcll(__ballot(lane >= SEQ_HELP_SLOTS && live));
		if (busy_l < cap_local && free_l) {
			const uint32_t slot = (uint32_t)__builtin_ctzll(free_l);
			if (lane == slot) {
				ws.rob[slot].px = qx; ws.rob[slot].py = qy; ws.rob[slot].lines_seen = post_seq;
				W_ST_REL(&ws.rob[slot].state, (uint32_t)H_POSTED);
				st = H_POSTED; spx = qx; spy = qy;
			}
			++post_seq;
		} else if (busy_r < cap_remote && free_r) desk_post_remote(ws, (uint32_t)__builtin_ctzll(free_r), qx, qy, st, spx, spy);
		else break;
	}
}

// owner, after a verdict that accepted no line: the posts that stand are still the scan's next survivors -- only an accepted
// line takes pixels out of the scan, and the pixel just visited left the desk in desk_take -- so all that is missing is one
// survivor further along.  Keeps `cap_local` posts on the workgroup's desk and `cap_remote` in the other workgroups' ring, going
// on from the cursor; a round with a full desk costs a state
// look.  `ahead` counts the survivors between the scan and the cursor: with none there, the next one found is the owner's own
// next candidate, which it casts itself (posted, it would arrive there a moment later, find it taken, and wait a whole cast).  (Looking the next survivors up from the dispatcher's position after EVERY verdict, as desk_refresh does, cost the
// owner 6.6 k cycles per round in the loaded pipeline: half of what its helpers saved it.)
__device__ __forceinline__ void desk_post_more(WShared &ws, const uint32_t *list, uint32_t *survw, uint32_t wy0, uint32_t wwords, int xorg, uint32_t cap_local, uint32_t cap_remote, uint32_t &post_seq,
                                               uint32_t &cur_e, int &cur_bit, uint32_t &ahead) {
	const uint32_t lane = opaque_lane();
	uint32_t st = H_DONE;
	if (lane < SEQ_DESK_ENTRIES) st = W_LD_ACQ(&ws.rob[lane].state);
	unsigned long long free_l = __ballot(lane < SEQ_HELP_SLOTS && st == (uint32_t)H_FREE);
	unsigned long long free_r = __ballot(lane >= SEQ_HELP_SLOTS && lane < SEQ_DESK_ENTRIES && st == (uint32_t)H_FREE);
	uint32_t busy_l = SEQ_HELP_SLOTS - (uint32_t)__popcll(free_l);
	uint32_t busy_r = (uint32_t)__popcll(__ballot(lane >= SEQ_HELP_SLOTS && lane < SEQ_DESK_ENTRIES && (st == (uint32_t)H_RPOSTED || st == (uint32_t)H_DONE)));
	// (cancelled posts a helper had taken hold their entries until the results are in: look when they are in the way)
	if (cap_remote && busy_r < cap_remote && !free_r && __ballot(lane >= SEQ_HELP_SLOTS && lane < SEQ_DESK_ENTRIES && st == (uint32_t)H_RZOMBIE)) {
		remote_harvest(ws);
		if (lane < SEQ_DESK_ENTRIES) st = W_LD_ACQ(&ws.rob[lane].state);
		free_r = __ballot(lane >= SEQ_HELP_SLOTS && lane < SEQ_DESK_ENTRIES && st == (uint32_t)H_FREE);
	}
	bool room_l = busy_l < cap_local && free_l, room_r = busy_r < cap_remote && free_r;
	if (!room_l && !room_r) return;
	const uint32_t n_lines = W_LD(&ws.n_lines), end = ws.disp_end, first = W_LD(&ws.disp_e);
	while ((room_l || room_r) && cur_e < end) {
		const uint32_t e0 = cur_e & ~63u;
		float fpx0, fpy;
		uint32_t w = disp_entry(ws, list, survw, e0 + lane, first, end, n_lines, wy0, wwords, xorg, fpx0, fpy);
		// (entries before the cursor's, and of the cursor's entry the bits up to the cursor's, have been looked at)
		if (e0 + lane < cur_e) w = 0u;
		else if (e0 + lane == cur_e && cur_bit >= 0) w = cur_bit >= 31 ? 0u : (w & ~((2u << (uint32_t)cur_bit) - 1u));
		const unsigned long long any = __ballot(w != 0u);
		if (!any) { cur_e = e0 + 64u; cur_bit = -1; continue; }
		const uint32_t src = (uint32_t)__builtin_ctzll(any);
		const uint32_t ww = (uint32_t)__builtin_amdgcn_readlane((int)w, (int)src);
		const uint32_t bit = (uint32_t)__builtin_ctz(ww);
		const uint32_t ppx = (uint32_t)((int)bcast_f(fpx0, src) + (int)bit), ppy = (uint32_t)bcast_f(fpy, src);
		cur_e = e0 + src; cur_bit = (int)bit;
		if (ahead++ == 0u) continue;                             // the owner's own next
		if (room_l) {
			const uint32_t slot = (uint32_t)__builtin_ctzll(free_l);
			free_l &= free_l - 1ull;
			if (lane == slot) {
				ws.rob[slot].px = ppx; ws.rob[slot].py = ppy; ws.rob[slot].lines_seen = post_seq;
				W_ST_REL(&ws.rob[slot].state, (uint32_t)H_POSTED);
			}
			++post_seq; ++busy_l;
		} else {
			uint32_t d0 = 0, d1 = 0, d2 = 0;
			desk_post_remote(ws, (uint32_t)__builtin_ctzll(free_r), ppx, ppy, d0, d1, d2);
			free_r &= free_r - 1ull;
			++busy_r;
		}
		room_l = busy_l < cap_local && free_l; room_r = busy_r < cap_remote && free_r;
	}
}

// dirs: the 3600 ray directions in LDS (a copy of g_ray_table).  TEAM: the frame may ask the other waves of its workgroup for
// help (the search service; tile store only).  REUSE: the wave's window block keeps its window between candidates (seq_cast_candidate)
// LEAN: seq_cast_candidate's
template <int MODE, bool WAVE = false, bool TEAM = false, bool REUSE = false, bool LEAN = false>
__device__ void lsd_frame_seq(const Geom &g, const Buffers &b, uint32_t f, float max_gap, const FrameAux &aux, uint32_t *smem, WShared &ws, const uint32_t *cull_tab, const RayDir *dirs,
                              uint32_t win_cap, uint32_t list_cap, const FrameView *tile_view = nullptr) {
	static_assert(!TEAM || (WAVE && (MODE == LSD_MODE_TILE || MODE == LSD_MODE_TILEC)), "helpers read the owner's tile store in LDS");
	const uint32_t lane = threadIdx.x & 63u;
	FrameView v;
	if constexpr (MODE == LSD_MODE_TILE || MODE == LSD_MODE_TILEC) v = *tile_view;
	else frame_setup<MODE, WAVE>(g, b, f, aux, smem, v);
	const Win &m = v.m;
	uint32_t *list = smem + win_cap, *survw = list + list_cap, *wwin = survw + list_cap;
	const uint32_t wy0 = v.wy0, wrows = v.wrows, wwords = v.wwords;
	const int xorg = v.xorg;
	const uint32_t WT = wrows * wwords;
	const uint32_t cull = cull_mode_for(b.cull_tab, max_gap);
	if (lane == 0) { ws.n_lines = 0u; ws.rounds = 0u; ws.steps = 0ull; }
	if (TEAM && lane < SEQ_DESK_ENTRIES) ws.rob[lane].state = H_FREE;
	if (TEAM && lane == 0) { ws.rem_open = 0u; ws.rem_nr = 0u; if (REUSE) ws.frame_no += 1u; }   // (frame_no: what a helper keys its window by, svc_help)
#ifdef SMH_LSD_WDEBUG
	if (lane < 8u) ws.dbg[lane] = 0u;
	if (lane < 10u) ws.rdbg[lane] = 0ull;
	if (lane == 0) ws.prof[0] = 0ull;
#endif
	const bool remote_ok = TEAM && ws.rem_r != 0ull;            // help across workgroups is on for this launch
	bool rem_open = false;
	uint32_t rem_nr = 0, rem_asked = 0;
	uint32_t rounds = 0, n_lines = 0, post_seq = 0;
	uint32_t seg_start = 0, cur_e = 0, ahead = 0;
	int cur_bit = -1;
	bool done = false, want = false, desk_valid = false;        // desk_valid: the posts and the cursor belong to this list and these lines
	// The window block holds nothing of THIS frame yet (the frame's set-up used it as scratch; the wave may have helped another
	// frame in it since its last own).  The mask does not change during the frame, so the tag stands until the frame ends.
	WinTag wtag = {0, 0, false};
#ifdef SMH_LSD_WDEBUG
	unsigned long long sprof[8] = {0, 0, 0, 0, 0, 0, 0, 0}, slast = __builtin_amdgcn_s_memtime(), uprof[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	uint32_t n_units = 0, n_taken = 0;
#define SPROF(i) do { const unsigned long long _n = __builtin_amdgcn_s_memtime(); sprof[i] += _n - slast; slast = _n; } while (0)
#else
#define SPROF(i)
#endif
	while (!done) {
		uint32_t segnext;
		const uint32_t n_list = seq_build_list<MODE>(m, ws, list, survw, list_cap, wy0, wrows, wwords, seg_start, WT, &segnext);
		if (lane == 0) { ws.disp_e = 0u; ws.disp_end = n_list; }
		desk_valid = false;
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
		SPROF(0);
		while (true) {
			uint32_t px = 0, py = 0;
			// lsd.rs:66-92: the next white pixel in raster order that lies near no accepted line
			if (!wave_dispatch(ws, list, survw, wy0, wwords, xorg, px, py)) break;
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");     // (lane 0's updates of the list state before the next look at it)
			__builtin_amdgcn_wave_barrier();
			SPROF(1);
			float xs = 0.0f, ys = 0.0f, ex0 = 0.0f, ey0 = 0.0f;
			unsigned long long wkey = 0ull;
			uint32_t st_sum = 0u;
			++rounds;
			if (ahead) --ahead;                                            // (the pixel the scan has arrived at)
			bool have = false;
#ifdef SMH_LSD_WDEBUG
			const unsigned long long t_tk = __builtin_amdgcn_s_memtime();
#endif
			if (TEAM && want) have = desk_take(ws, px, py, xs, ys, wkey, ex0, ey0, st_sum);
#ifdef SMH_LSD_WDEBUG
			if (rem_open) RDBG(7, __builtin_amdgcn_s_memtime() - t_tk);
#endif
#ifdef SMH_LSD_WDEBUG
			if (have) ++n_taken;
			if (!have) seq_cast_candidate<MODE, REUSE, LEAN>(m, wwin, &wtag, cull_tab, cull, dirs, b.ray_off, max_gap, px, py, xs, ys, wkey, ex0, ey0, st_sum, sprof, slast, uprof, n_units);
#else
			if (!have) seq_cast_candidate<MODE, REUSE, LEAN>(m, wwin, &wtag, cull_tab, cull, dirs, b.ray_off, max_gap, px, py, xs, ys, wkey, ex0, ey0, st_sum);
#endif
			if (lane == 0) ws.steps += st_sum;
			if (wkey != 0ull && __uint_as_float((uint32_t)(wkey >> 32)) > SMH_LSD_ACCEPT_LEN_SQ) {   // lsd.rs:94
				float ex, ey;
				get_centre(m, ex0, ey0, ex, ey);                            // lsd.rs:96-99: the far end is centred too
				if (lane == 0) {
					ws.lines[n_lines][0] = xs; ws.lines[n_lines][1] = ys; ws.lines[n_lines][2] = ex; ws.lines[n_lines][3] = ey;
					const ProxLine pl = prox_line(xs, ys, ex, ey);
					ws.prox_a[n_lines] = pl.a; ws.prox_d[n_lines][0] = pl.dxl; ws.prox_d[n_lines][1] = pl.dyl;
					W_ST_REL(&ws.n_lines, n_lines + 1u);
				}
				++n_lines;
				desk_valid = false;                                         // the survivors behind this pixel have changed
				__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
				__builtin_amdgcn_wave_barrier();
				__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
				if (n_lines == SMH_LSD_MAX_LINES) { done = true; break; }   // lsd.rs:101-103
			}
			if (TEAM) {
				if (!want && rounds >= SEQ_HELP_AFTER) {
					want = true;
					if (lane == 0) W_ST_REL(&ws.want_set, 1u);
				}
				if (want) {
					// a frame that is still at work after `rem_after` rounds asks the other workgroups as well (looked at every
					// fourth round: a look at the request's state word is a round trip to memory)
					// a frame that is still at work after `rem_after` rounds AND is among the last of its submission -- what keeps a
					// submission's slot busy is its slowest frames -- asks the other workgroups as well (looked at every other round:
					// a look at a word in memory is a round trip)
					if (remote_ok && (rounds & (rem_open ? 7u : 1u)) == 0u) {
						if (rem_open) {
							rem_nr = remote_helpers(ws);
							// helpers come and go (a helper that finds nothing to take for a while goes back to frames of its own): the
							// frame asks again while fewer than it wanted are there
							const uint32_t want_h = uniform_u32(ws.rem_tickets);
							if (rem_nr * 2u < want_h && rounds - rem_asked >= 8u) {
								if ((ws.rem_flags & 1u) || (int32_t)uniform_u32((uint32_t)__hip_atomic_load(&rem_ctl_of(ws)->avail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) <= 0)
									(void)remote_issue_tickets(ws, rem_ctl_of(ws), uniform_u32(ws.rem_gen), want_h - rem_nr);
								rem_asked = rounds;
							}
						}
						else if (rounds >= uniform_u32(ws.rem_after) && ws.disp_end - min(W_LD(&ws.disp_e), ws.disp_end) >= SEQ_REMOTE_MIN_LEFT) {
							const uint32_t *dp = (const uint32_t *)(uintptr_t)(((unsigned long long)uniform_u32((uint32_t)(ws.rem_done >> 32)) << 32) | uniform_u32((uint32_t)ws.rem_done));
							const uint32_t n_sub = uniform_u32(ws.rem_n), fin = uniform_u32(__hip_atomic_load(dp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
							// ... and only while no frame is waiting for a wave: a wave that helps then is a wave that would have slept
							const bool free_waves = (ws.rem_flags & 1u) || (int32_t)uniform_u32((uint32_t)__hip_atomic_load(&rem_ctl_of(ws)->avail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) <= 0;
							if (free_waves && (n_sub - min(fin, n_sub)) * uniform_u32(ws.rem_last_div) <= n_sub) rem_asked = rounds;
#ifdef SMH_LSD_WDEBUG
							if (rem_asked == rounds && lane == 0) { ws.dbg[3] += 1u; if (ws.dbg[4] == 0u) ws.dbg[4] = rounds; }
#endif
							if (rem_asked == rounds)
								rem_open = remote_open<MODE == LSD_MODE_TILEC>((uint32_t)(uintptr_t)(const LdsByte *)&ws, (uint32_t)(uintptr_t)(const LdsByte *)smem, MODE == LSD_MODE_TILEC ? tilec_idx_words(g.rw, g.rh) : tile_idx_words(g.rw, g.rh));
						}
					}
					const uint32_t nh = uniform_u32(W_LD(&ws.late));       // helpers of the workgroup attached
					// (one post per helper here; two where an answer takes microseconds -- and two from the moment the request opens, so that the
					// first helper to arrive finds work)
					const uint32_t cap_l = min(nh, SEQ_HELP_SLOTS - 1u), cap_r = rem_open ? min(2u + 2u * rem_nr, SVC_REMOTE_RING) : 0u;
					if (!cap_l && !cap_r) desk_valid = false;
					else if (!desk_valid) {
#ifdef SMH_LSD_WDEBUG
						const unsigned long long t_r = __builtin_amdgcn_s_memtime();
#endif
						desk_refresh(ws, list, survw, wy0, wwords, xorg, cap_l, cap_r, post_seq, cur_e, cur_bit, ahead);   // (its own next + the posts)
						desk_valid = true;
#ifdef SMH_LSD_WDEBUG
						if (rem_open) { RDBG(3, 1ull); RDBG(5, __builtin_amdgcn_s_memtime() - t_r); }
#endif
					} else {
#ifdef SMH_LSD_WDEBUG
						const unsigned long long t_r = __builtin_amdgcn_s_memtime();
#endif
						desk_post_more(ws, list, survw, wy0, wwords, xorg, cap_l, cap_r, post_seq, cur_e, cur_bit, ahead);
#ifdef SMH_LSD_WDEBUG
						if (rem_open) RDBG(6, __builtin_amdgcn_s_memtime() - t_r);
#endif
					}
#ifdef SMH_LSD_WDEBUG
					if (rem_open) { RDBG(8, 1ull); if (lane == 0 && ws.rdbg[9] == 0ull) ws.rdbg[9] = __builtin_amdgcn_s_memtime(); }
#endif
				}
			}
			SPROF(4);
		}
		if (segnext >= WT) break;
		seg_start = segnext;
	}
	if (TEAM) {
		// the helpers read this frame's mask tiles: they have left before the wave goes on to its next frame
		if (lane == 0) W_ST_REL(&ws.want_set, 0u);
		if (rem_open) remote_close(ws);
		while (uniform_u32(W_LD_ACQ(&ws.late)) != 0u) __builtin_amdgcn_s_sleep(2);
	}
	smhv_frame_result *res = &b.results[f];
	if (lane < n_lines) {
		res->lines[lane].x0 = ws.lines[lane][0]; res->lines[lane].y0 = ws.lines[lane][1];
		res->lines[lane].x1 = ws.lines[lane][2]; res->lines[lane].y1 = ws.lines[lane][3];
	}
	if (lane == 0) { res->n_lines = n_lines; res->rounds = rounds; res->ray_steps = ws.steps; res->status = SMHV_FRAME_OK; }
#ifdef SMH_LSD_WDEBUG
	// diagnostic build only: cycles of list build, dispatch, set-up, units, verdict (+ the desk); inside the units: first batches,
	// long rays, end points; units cast; candidates taken from the desk (never read by product code in that build)
	if (lane == 0) {
		for (int k = 0; k < 5; ++k) res->meters[20 + k] = (double)sprof[k];
		for (int k = 0; k < 3; ++k) res->meters[25 + k] = (double)uprof[8 + k];
		res->meters[30] = (double)uprof[0]; res->meters[31] = (double)uprof[1];   // inside set-up: window fill, culling scan
		res->length_px[28] = (double)uprof[2];                                    // window fills of the owner (candidates cast here minus windows reused)
		res->meters[28] = (double)n_units;
		res->meters[29] = (double)n_taken;
		// help across workgroups: arrivals at remote posts, taken back, waited for (and for how many cycles), requests opened, round of the request
		res->length_px[22] = (double)ws.dbg[0]; res->length_px[23] = (double)ws.dbg[1]; res->length_px[24] = (double)ws.dbg[2]; res->length_px[25] = (double)ws.prof[0];
		res->length_px[26] = (double)ws.dbg[3]; res->length_px[27] = (double)ws.dbg[4];
		// ... with the request open (the record tail of this build leaves angle[16..] alone): posts, cancelled free / taken, refreshes, harvests, cycles in refresh /
		// post_more / take, rounds; cycles since the request opened
		for (int k = 0; k < 9; ++k) res->angle[16 + k] = (float)ws.rdbg[k];
		res->angle[25] = ws.rdbg[9] ? (float)(__builtin_amdgcn_s_memtime() - ws.rdbg[9]) : 0.0f;
	}
#endif
}
