// smh_lsd_wave.inc -- k_lsd_tile: lsd::find_lines::<32> as tasks instead of barriers, on a sparse tile store of the mask
// (included by smh_lsd.hip; the default line search since round 2).
//
// k_lsd (above) casts a group of candidates with the whole workgroup in lock step: nine barriers per group, and every
// phase of a group runs at the pace of its slowest wave.  Here the waves of a frame's workgroup run on their own:
//   * candidates (surviving white pixels in raster order) sit in a reorder buffer; an idle wave claims one 64-ray UNIT of the
//     oldest candidate that still has one and does everything that unit needs -- the first two batches of every ray, the
//     long rays to their end, the exact end points that can matter -- with wave-level reductions only;
//   * results retire IN ORDER: a candidate is resolved (round counted, line accepted, ...) only when every candidate
//     dispatched before it has been, exactly as the sequential scan would have met them.  A candidate that turns out to
//     lie near a line accepted after it was dispatched is dropped at that point (the sequential scan would never have
//     visited it);
//   * survivor words are filtered against new lines lazily, when the dispatcher next looks at them.
// Dispatch and retirement are serialised by one LDS try-lock.  Casting a candidate is a pure function of (mask, pixel), so
// lines, round counts and sample counts are those of the sequential reference bit for bit -- the same argument as for the
// speculative groups of k_lsd.
// The mask is held as its non-empty 32 x 8 px tiles plus a 16-bit index (LSD_MODE_TILE, frame_setup_tile below): 20-50 KB
// for any frame size where k_lsd needs 110 KB at 1080p and a sliding row cache beyond.  Vision::find_longest_line (57 units
// of ONE candidate) and batches run with helper workgroups stay on k_lsd.

#ifndef W_WAVES_PER_EU
#define W_WAVES_PER_EU 4                // 128 VGPRs: three 123-register waves of the streaming pass still fit beside one of these per SIMD
#endif
#ifndef W_A_BATCHES
#define W_A_BATCHES LSD_A_BATCHES       // 32-sample batches every ray of a unit is walked for before the survivors are treated as long rays
#endif
#ifndef W_NWIN
#define W_NWIN 4u                       // candidates in flight (one window each)
#endif
#define W_ROB 16u                       // reorder buffer entries (candidates in flight, local and remote, + waiting to retire): a power of two
#define W_LIST_CAP_MAX 1024u            // non-zero mask words per segment of the raster scan (launch parameter list_cap <= this; the scan continues
                                        // segment by segment, and every segment boundary drains the candidates in flight)
// Candidate windows (LSD_MODE_WIN2, smh_lsd.hip): the first W_A_BATCHES x 32 steps of a ray stay within 64 px of its start
// point, which get_centre puts within 2.5 px of the candidate's pixel.  W_WIN_R rows / columns on either side of the pixel,
// columns rounded down to a word: LSD_W2_PITCH words.  One window per candidate in flight: slot s uses window s % W_NWIN, and
// at most W_NWIN candidates are in flight (the speculation width stops there: measured, wider buys nothing).
#define W_WIN_R 67
#define W_WIN_ROWS (2 * W_WIN_R + 1)
#include "smh_window_place.h"
static_assert(W_WIN_R == SMH_WIN_R && LSD_W2_PITCH == SMH_WIN_WORDS, "smh_window_place.h speaks of this window");
#define W_WIN_STRIDE (W_WIN_ROWS * LSD_W2_PITCH + 2u)   // words per window (+2: the culling scan's funnel shift reads one word past a row's end)
#ifndef W_SPEC_MAX
#define W_SPEC_MAX 8u                   // candidates between dispatch and retirement (W_NWIN of them being cast, the others waiting for their turn to retire)
#endif
static_assert(W_SPEC_MAX + SMH_FARM_RING <= W_ROB && W_NWIN <= W_SPEC_MAX && W_NWIN + SMH_FARM_RING <= W_ROB && (W_ROB & (W_ROB - 1u)) == 0u && W_NWIN <= 32u, "reorder buffer: every local (one window each) and remote (one ring entry each) candidate in flight has a slot");
static_assert(2 * W_WIN_R + 1 + 31 <= 32 * LSD_W2_PITCH, "a window row holds the neighbourhood from a word boundary on");
static_assert(W_WIN_R >= 32 * (int)W_A_BATCHES + 3 && W_WIN_R >= SMH_SECTOR_R + 3, "the window covers the first batches and the culling annulus");
#ifndef W_SPEC_MIN
#define W_SPEC_MIN 2u                   // candidates in flight right after an acceptance (doubles with every candidate retired without one)
#endif
#ifndef W_SPEC_GROW
#define W_SPEC_GROW(s) ((s) * 2u)
#endif
#define W_SPIN_LIMIT_DEFAULT 4000000u   // idle polls of one wave (~0.25 us each) before the watchdog gives the frame up (launch parameter)

struct WSlot {
	uint32_t px, py;                    // candidate pixel
	uint32_t lines_seen;                // accepted lines when it was dispatched
	uint32_t state;                     // W_FREE / W_SETUP / W_CASTING / W_DONE
	float ptx, pty;                     // get_centre of the pixel = start point of its rays
	unsigned long long todo;            // 64-ray units nobody has claimed yet
	unsigned long long live;            // all units that have to be cast (sector culling)
	unsigned long long best;            // max over the exactly evaluated rays of (len^2 bits << 32 | ray index) ...
	float ex, ey;                       // ... and that ray's end point (updated under `block`)
	uint32_t block;
	uint32_t pending;                   // units not merged yet; the wave that brings it to 0 finishes the candidate
	uint32_t steps;                     // mask samples of all rays
	uint32_t win;                       // local candidate: its window; remote candidate (cast by the frame's helper workgroup): its ring entry
	unsigned long long tag;             // remote: the `done` tag its result will carry
#ifdef SMH_LSD_WDEBUG
	unsigned long long t_disp, t_setup, t_done;   // dispatched; set up (units published); last unit merged
#endif
};
enum { W_FREE = 0, W_SETUP = 1, W_CASTING = 2, W_DONE = 3, W_REMOTE = 4 };

struct WShared {
	WSlot rob[W_ROB];
	uint32_t lock;
	uint32_t head, tail;                // candidates retired / dispatched
	uint32_t spec;                      // candidates allowed in flight
	uint32_t disp_e, disp_end;          // next list entry the dispatcher looks at; entries in the chunk
	uint32_t n_lines, rounds, frame_done;
	unsigned long long steps;
	float lines[SMH_LSD_MAX_LINES][4];
	float prox_a[SMH_LSD_MAX_LINES];
	double prox_d[SMH_LSD_MAX_LINES][2];
	unsigned char stag[W_LIST_CAP_MAX];   // lines already applied to a list entry's survivor word
	uint32_t scan[LSD_NW];
	uint32_t segnext;
	uint32_t ntiles;                    // LSD_MODE_TILE: non-empty tiles found while building the tile store
	uint32_t stuck;                     // watchdog
	uint32_t win_free;                  // windows nobody uses (bit mask)
	uint32_t farm_on, farm_posted, farm_retired, frame_no;   // helper exchange: helper attached; candidates posted / retired; (the search service:) frames this block's wave has begun
	uint32_t late, want_set, want_tick, pick;                 // late helpers: mode; the frame has asked for help; retirements since the last refresh; (target choice)
	unsigned long long t0, late_cycles;                        // s_memtime when the search of the frame began; how long it works alone before it asks
	// the search service's help across workgroups (smh_lsd_seq.inc, "the desk across workgroups"): set once per wave by the kernel ...
	unsigned long long rem_r, rem_store, rem_ctl;              // this wave's SvcRemote, its block of SvcParams::remote_store, the service's SvcCtl (0: no such help)
	uint32_t rem_after, rem_tickets, rem_owner, rem_cap;       // SvcParams::remote_after / remote_tickets, workgroup * waves + wave, tile_cap
	// ... and per frame by its owner
	uint32_t rem_open, rem_gen, rem_k, rem_nr;                 // a request is open; its number; posts so far; helpers attached when last looked
	unsigned long long rem_done;                               // address of the frame's submission's count of finished frames (SvcSlot::done), and ...
	uint32_t rem_n, rem_last_div;                              // ... its frames: a frame asks once it is among the last 1 / rem_last_div of its submission
	uint32_t rem_flags, rem_pad;                               // 1: ask whether or not frames are waiting for a wave
#ifdef SMH_LSD_WDEBUG
	uint32_t dbg[8];
	unsigned long long rdbg[10];        // the desk across workgroups: posts issued, cancelled (free at once / a helper had it), refreshes, harvests, cycles in refresh / post_more / take, rounds with the request open, when it opened
	uint32_t why[4];                    // an idle wave found no dispatch possible because of: the speculation width, no free window, list exhausted; (polls in all)
	unsigned long long prof[12];        // wave-cycles: claim, unit, finish, lock wait, control, setup, idle, total; inside unit: first batches, long rays, end points, merge
	unsigned long long lat[8];          // dispatch -> retire latency: sum for accepted, count, sum for rejected, count; local candidates: sum dispatch -> set up, set up -> last unit merged, merged -> retired, count
#endif
};
#ifdef SMH_LSD_WDEBUG
#define WDBG(i, v) do { if ((threadIdx.x & 63u) == 0) atomicAdd(&ws.dbg[i], (v)); } while (0)
#define WPROF(i) do { const unsigned long long _n = __builtin_amdgcn_s_memtime(); wprof[i] += _n - wlast; wlast = _n; } while (0)
#else
#define WDBG(i, v)
#define WPROF(i)
#endif

#define W_LD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define W_LD_ACQ(p) __hip_atomic_load((p), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)
#define W_ST(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define W_ST_REL(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP)

__device__ __forceinline__ float bcast_f(float v, uint32_t src) { return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), (int)src)); }
__device__ __forceinline__ uint32_t uniform_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// The window of the candidate whose pixel is (px, py), in the LDS block `wwin`: -> m.w2 (byte address of image word (0, 0)).
__device__ __forceinline__ const LdsByte *window_base(const uint32_t *wwin, uint32_t px, uint32_t py) {
	const int x0 = ((int)px - W_WIN_R) & ~31, y0 = (int)py - W_WIN_R;
	return (const LdsByte *)(const LdsWord *)wwin - (__mul24(y0, (int)(4u * LSD_W2_PITCH)) + ((x0 >> 5) << 2));
}
// ... and of the window placed at word column x0w, row y0
__device__ __forceinline__ const LdsByte *window_base_at(const uint32_t *wwin, int x0w, int y0) {
	return (const LdsByte *)(const LdsWord *)wwin - (__mul24(y0, (int)(4u * LSD_W2_PITCH)) + (x0w << 2));
}
// Where the window in a block lies (the search service: one wave, one block, one candidate after the other).  The scan visits
// white pixels in raster order and its rejected candidates are neighbours, so the next candidate nearly always needs words that
// are already there: cand_setup fills the block only when its rectangle no longer contains what the candidate reads
// (smh_window_place.h) and places every reader through the tag.  Wave-uniform; lives in the caller's scalar registers.
// Whoever owns the tag clears `valid` whenever the mask store the window was filled from may have changed.
struct WinTag { int x0w, y0; bool valid; };
// A freshly dispatched candidate: its window (copied from the frame's mask store), get_centre (lsd.rs:5-44) of its pixel,
// then the sector culling scan -> ptx, pty, live.  `wwin`: the candidate's window block (W_WIN_STRIDE words).
// (lane ids are made opaque at the start of every per-candidate phase: the compiler otherwise hoists two dozen lane-derived
// index constants out of the candidate loop and spills them -- and a spill reload is a vector-memory access, which beside the
// HBM-bound streaming pass takes microseconds)
__device__ __forceinline__ uint32_t opaque_lane() { uint32_t l = threadIdx.x & 63u; asm volatile("" : "+v"(l)); return l; }
// TAGGED with `tag` (neither: k_lsd_tile's shared windows, filled for every candidate): the block's window may serve as it lies.  ROWS: the
// rows a fill covers, from py - W_WIN_R on (the service's taller window: rows BELOW the needed region, for the scan's next rows).
template <bool COMPACT = false, uint32_t ROWS = W_WIN_ROWS, bool TAGGED = false>
__device__ __forceinline__ void cand_setup(const Win &m, uint32_t *wwin, const uint32_t *cull_tab, uint32_t cull, uint32_t px, uint32_t py, float &xs, float &ys, unsigned long long &live,
                                           WinTag *tag = nullptr
#ifdef SMH_LSD_WDEBUG
                                           , unsigned long long *cprof = nullptr                       // [0] window fill, [1] culling scan (cycles), [2] window fills
#endif
                                           ) {
	static_assert(ROWS >= W_WIN_ROWS, "a fill covers its own candidate's needed rows");
	const uint32_t lane = opaque_lane();
#ifdef SMH_LSD_WDEBUG
	const unsigned long long c_t0 = __builtin_amdgcn_s_memtime();
#endif
	[[maybe_unused]] bool fill = true;
	if constexpr (TAGGED) {                                         // (the pixel is wave-uniform: the tag stays in scalar registers)
		const int upx = (int)uniform_u32(px), upy = (int)uniform_u32(py);
		if (tag->valid && smh_window_holds(tag->x0w, tag->y0, (int)ROWS, upx, upy)) fill = false;
		else { smh_window_fresh(upx, upy, &tag->x0w, &tag->y0); tag->valid = true; }
	}
	if (!TAGGED || fill) {
		const int wq0 = TAGGED ? tag->x0w : (((int)px - W_WIN_R) & ~31) >> 5, y0 = TAGGED ? tag->y0 : (int)py - W_WIN_R;
		constexpr uint32_t NIT = (ROWS * LSD_W2_PITCH + 63u) / 64u;
		if (m.tiled) {
			// A marker mask is 1-4 % non-empty: of the 18 x 6 tiles under a window a handful hold a set bit.  So: the window is
			// zeroed (stores, nothing to wait for), the index entries of the tiles under it are read in ONE round trip (two per
			// lane), and the non-empty tiles are copied eight at a time (eight lanes per tile, one row each).  Looking every
			// one of the window's 810 words up through the index -- two dependent LDS reads per word, thirteen rounds -- was
			// 7 k cycles per candidate in the loaded pipeline.
#pragma unroll
			for (uint32_t k = 0; k < NIT; ++k) {
				const uint32_t i = lane + 64u * k;
				if (i < ROWS * LSD_W2_PITCH) wwin[i] = 0u;
			}
			const int ty0 = y0 >> 3, ty1 = (y0 + (int)ROWS - 1) >> 3;     // (arithmetic shifts: rows above the image are negative)
			const uint32_t nslots = (uint32_t)(ty1 - ty0 + 1) * LSD_W2_PITCH;   // <= 18 x 6 = 108 = two per lane (135 rows; 159 rows: 21 x 6 = 126)
			static_assert(((ROWS + 6u) / 8u + 1u) * LSD_W2_PITCH <= 128u, "two tile slots per lane cover the window (ROWS rows from any row of a tile on touch at most (ROWS + 6) / 8 + 1 tile rows)");
			uint32_t tv[2];
#pragma unroll
			for (uint32_t rnd = 0; rnd < 2u; ++rnd) {
				const uint32_t sidx = lane + 64u * rnd, tr = sidx / LSD_W2_PITCH, tc = sidx - tr * LSD_W2_PITCH;
				const int ty = ty0 + (int)tr, wq = wq0 + (int)tc;
				const bool ok = sidx < nslots && ty >= 0 && (uint32_t)(ty << 3) < m.h && (uint32_t)(wq + 2) < m.t_pitch;
				if constexpr (COMPACT) tv[rnd] = ok ? tilec_number(m, wq, ty) : 0u;
				else tv[rnd] = ok ? (uint32_t)m.t_idx[__mul24(ty, (int)m.t_pitch) + wq] : 0u;   // (0: the empty tile)
			}
			const uint32_t grp = lane >> 3, row = lane & 7u;
#pragma unroll
			for (uint32_t rnd = 0; rnd < 2u; ++rnd) {
				unsigned long long todo = __ballot(tv[rnd] != 0u);
				while (todo) {
					uint32_t src = 64u;                                 // the lane that holds this lane group's tile (64: none)
#pragma unroll
					for (uint32_t k = 0; k < 8u; ++k) {
						const uint32_t p = todo ? (uint32_t)__builtin_ctzll(todo) : 64u;
						todo &= todo - 1ull;                            // (0 stays 0)
						if (grp == k) src = p;
					}
					const uint32_t tt = (uint32_t)__shfl((int)tv[rnd], (int)(src & 63u));
					const uint32_t sidx = src + 64u * rnd, tr = sidx / LSD_W2_PITCH, tc = sidx - tr * LSD_W2_PITCH;
					const int rr = ((ty0 + (int)tr) << 3) + (int)row - y0;      // the window row this lane's tile row lands in
					if (src < 64u && rr >= 0 && rr < (int)ROWS) wwin[(uint32_t)rr * LSD_W2_PITCH + tc] = (uint32_t)m.t_tiles[(tt << 3) + row];
				}
			}
		} else {
#pragma unroll 1
			for (uint32_t i = lane; i < ROWS * LSD_W2_PITCH; i += 64u) {
				const uint32_t r = i / LSD_W2_PITCH, c = i - r * LSD_W2_PITCH;
				const int b0 = ((wq0 + (int)c) << 5) + m.xbias;             // (the global rows start xbias bits left of pixel 0)
				wwin[i] = __builtin_amdgcn_alignbit(win_word(m, (b0 >> 5) + 1, y0 + (int)r), win_word(m, b0 >> 5, y0 + (int)r), (uint32_t)b0 & 31u);
			}
		}
		if (lane < 2u) wwin[ROWS * LSD_W2_PITCH + lane] = 0u;
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");        // this wave reads the window next; the others after the release of `todo`
		__builtin_amdgcn_wave_barrier();
	}
#ifdef SMH_LSD_WDEBUG
	if (cprof) { cprof[0] += __builtin_amdgcn_s_memtime() - c_t0; if (fill) cprof[2] += 1ull; }
#endif
	Win mw = m;
	mw.w2 = TAGGED ? window_base_at(wwin, tag->x0w, tag->y0) : window_base(wwin, px, py);
	{   // lane (dir, k) evaluates the k-th loop condition of direction dir (left, right, up, down)
		const uint32_t l = lane & 31u, dir = l >> 3, k = l & 7u;
		const float cx = (float)px, cy = (float)py, fk = (float)k;
		bool cond = k < 5u;                                           // (pixels within 4 of the candidate's: inside the window)
		if (dir == 0u) cond = cond && (cx - fk > 0.0f);
		else if (dir == 1u) cond = cond && (cx + fk < (float)(m.w - 1u));
		else if (dir == 2u) cond = cond && (cy - fk > 0.0f);
		else cond = cond && (cy + fk < (float)(m.h - 1u));
		if (cond) {
			const int k_ = (int)k;
			const int xi = (int)px + (dir == 0u ? -k_ : (dir == 1u ? k_ : 0)), yi = (int)py + (dir == 2u ? -k_ : (dir == 3u ? k_ : 0));
			cond = win2_bit(mw, xi, yi) != 0u;
		}
		const uint32_t bits = (uint32_t)__ballot(cond);
		const float nl = (float)__builtin_ctz(~(bits & 0xFFu)), nr = (float)__builtin_ctz(~((bits >> 8) & 0xFFu));
		const float nu = (float)__builtin_ctz(~((bits >> 16) & 0xFFu)), nd = (float)__builtin_ctz(~((bits >> 24) & 0xFFu));
		xs = ((cx - nl) + (cx + nr)) / 2.0f;
		ys = ((cy - nu) + (cy + nd)) / 2.0f;
	}
	live = (1ull << LSD_GROUPS) - 1ull;
#ifdef SMH_LSD_WDEBUG
	const unsigned long long c_t1 = __builtin_amdgcn_s_memtime();
	struct CullTimer { unsigned long long *p, t; __device__ ~CullTimer() { if (p) p[1] += __builtin_amdgcn_s_memtime() - t; } } c_timer{cprof, c_t1};
#endif
	if (cull) {   // the 64-ray units that can see a white pixel in the outer annulus (chained: and one in the middle annulus; smh_cull_rule.h)
		const int fx = (int)floorf(xs), fy = (int)floorf(ys);
		// One wave per SIMD has nobody else to hide an LDS round trip behind, so the window words and the cell masks of all
		// seven cell rounds are read in ONE.  No branch per round (each would get a wait of its own): a lane past the last cell
		// takes the last cell again, and what it finds there is ORed in a second time.
		constexpr int ROUNDS = (SMH_CULL_CELLS + 63) / 64;
		const uint32_t sh = (uint32_t)(fx - SMH_SECTOR_R) & 31u;        // (the same for every cell: their columns are 32 apart)
		uint32_t cells[ROUNDS], lo[ROUNDS], hi[ROUNDS], m_out[ROUNDS], m_mid[ROUNDS];
#pragma unroll
		for (int it = 0; it < ROUNDS; ++it) {
			const uint32_t cell = 64 * it + 63 < SMH_CULL_CELLS ? lane + 64u * (uint32_t)it : min(lane + 64u * (uint32_t)it, (uint32_t)SMH_CULL_CELLS - 1u);
			const int yi = fy + (int)(cell >> 2) - SMH_SECTOR_R;        // (rows outside the image are zero in the window)
			const int wq = (fx - SMH_SECTOR_R + (int)((cell & 3u) << 5)) >> 5;
			lo[it] = win2_word(mw, wq, yi); hi[it] = win2_word(mw, wq + 1, yi);
			m_out[it] = cull_tab[cell]; m_mid[it] = SMH_CULL_MID_CELL(cull_tab, cell);
			cells[it] = cell;
		}
		// The white annulus pixels' unit codes, a byte each in LDS.  A lane takes its cells' pixels by RUNS (smh_cull_rule.h: the
		// units of a run are the interval about the codes of its two ends; an annulus the run rule does not hold for: every
		// pixel a run of its own), the outer and the middle annulus' apart -- a pixel can lie in both.  A marker line leaves a
		// cell one run per annulus, so the first run of either annulus of all seven cells is looked up in ONE round trip, four
		// look-ups per cell; a lane without a run looks its cell's first pixel up and drops it.  The cells that hold more runs
		// are walked after that, a run of either annulus per round trip, and the wave waits for the lane with the most.
		// (-DSMH_CULL_CHAIN: the middle annulus' runs double the interval arithmetic below, which costs more than the units the
		// chain saves -- as the walk of both annuli pixel by pixel did: DESIGN.md section 5.)
		const uint8_t *codes = SMH_CULL_CODES(cull_tab);
		const bool chained = (cull & SMH_CULL_MODE_RULE) == 2u, runs_o = (cull & SMH_CULL_MODE_RUNS_OUTER) != 0u, runs_m = (cull & SMH_CULL_MODE_RUNS_MIDDLE) != 0u;
		unsigned long long acc_o = 0ull, acc_m = 0ull;
		uint32_t s_o[ROUNDS], e_o[ROUNDS], s_m[ROUNDS], e_m[ROUNDS], code[ROUNDS][4];
#pragma unroll
		for (int it = 0; it < ROUNDS; ++it) {
			const uint32_t px32 = __builtin_amdgcn_alignbit(hi[it], lo[it], sh);   // the cell's 32 pixels
			const uint32_t h_out = px32 & m_out[it], h_mid = chained ? px32 & m_mid[it] : 0u;
			s_o[it] = smh_cull_run_starts(h_out, runs_o); e_o[it] = smh_cull_run_ends(h_out, runs_o);
			s_m[it] = smh_cull_run_starts(h_mid, runs_m); e_m[it] = smh_cull_run_ends(h_mid, runs_m);
			const uint8_t *c = codes + (cells[it] >> 2) * SMH_SECTOR_DIM + ((cells[it] & 3u) << 5);
			code[it][0] = c[s_o[it] ? (uint32_t)__builtin_ctz(s_o[it]) : 0u]; code[it][1] = c[e_o[it] ? (uint32_t)__builtin_ctz(e_o[it]) : 0u];
			code[it][2] = c[s_m[it] ? (uint32_t)__builtin_ctz(s_m[it]) : 0u]; code[it][3] = c[e_m[it] ? (uint32_t)__builtin_ctz(e_m[it]) : 0u];
		}
		uint32_t more = 0u;
#pragma unroll
		for (int it = 0; it < ROUNDS; ++it) {
			if (s_o[it]) acc_o |= smh_cull_run_units(code[it][0], code[it][1]);
			if (s_m[it]) acc_m |= smh_cull_run_units(code[it][2], code[it][3]);
			s_o[it] &= s_o[it] - 1u; e_o[it] &= e_o[it] - 1u;               // (0 stays 0)
			s_m[it] &= s_m[it] - 1u; e_m[it] &= e_m[it] - 1u;
			more |= s_o[it] | s_m[it];
		}
		if (__any(more != 0u)) {                                        // (uniform) a cell with two runs of one annulus: two lines side by side, a dotted one
#pragma unroll
			for (int it = 0; it < ROUNDS; ++it) {
				const uint8_t *c = codes + (cells[it] >> 2) * SMH_SECTOR_DIM + ((cells[it] & 3u) << 5);
				uint32_t so = s_o[it], eo = e_o[it], sm = s_m[it], em = e_m[it];
				while (so | sm) {
					const uint32_t c0 = c[so ? (uint32_t)__builtin_ctz(so) : 0u], c1 = c[eo ? (uint32_t)__builtin_ctz(eo) : 0u];
					const uint32_t c2 = c[sm ? (uint32_t)__builtin_ctz(sm) : 0u], c3 = c[em ? (uint32_t)__builtin_ctz(em) : 0u];
					if (so) acc_o |= smh_cull_run_units(c0, c1);
					if (sm) acc_m |= smh_cull_run_units(c2, c3);
					so &= so - 1u; eo &= eo - 1u; sm &= sm - 1u; em &= em - 1u;
				}
			}
		}
		const unsigned long long seen_outer = cull_fold(wave_or64(acc_o));
		live = chained ? smh_cull_live(seen_outer, cull_fold(wave_or64(acc_m)), true) : seen_outer;
	}
}

// merge a wave's best exactly evaluated ray into the candidate (keys are unique per ray).  All 64 lanes active.
__device__ __forceinline__ void slot_merge_best(WSlot &sl, unsigned long long key, float xe, float ye) {
	if (!__any(key != 0ull)) return;                            // most units hold no ray that needs its end point
	// max of the 64-bit keys as two DPP reductions (no LDS round trips): the length bits, then the ray index among the longest
	const uint32_t hi = (uint32_t)(key >> 32), lo = (uint32_t)key;
	const uint32_t mhi = wave_max32_dpp(hi);
	const uint32_t mlo = wave_max32_dpp(hi == mhi ? lo : 0u);
	const unsigned long long wkey = ((unsigned long long)mhi << 32) | mlo;
	if (wkey == 0ull) return;                                   // uniform
	const uint32_t src = (uint32_t)__builtin_ctzll(__ballot(key == wkey));
	const float bx = bcast_f(xe, src), by = bcast_f(ye, src);
	if ((threadIdx.x & 63u) == 0u) {
		while (__hip_atomic_exchange(&sl.block, 1u, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != 0u) __builtin_amdgcn_s_sleep(1);
		if (wkey > sl.best) { sl.best = wkey; sl.ex = bx; sl.ey = by; }
		__hip_atomic_store(&sl.block, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
	}
}

// 32 consecutive samples of a ray whose batch starts with the offsets (xo, yo): whiteness bits (sample j -> bit j) and the
// number n of leading in-image samples (positions are monotonic along a ray, so the in-image samples are a prefix).  A
// batch that starts outside the image is not sampled at all (a ray never re-enters; and only a batch that starts inside
// stays within the 33 px the row window's padding absorbs).
template <int MODE>
__device__ __forceinline__ void sample32(const Win &m, float xs, float ys, float dx, float dy, float xo, float yo, uint32_t &Wm, uint32_t &n) {
	Wm = 0u; n = 0u;
	if (!in_image(m, xo + xs, yo + ys)) return;
	const float xo0 = xo, yo0 = yo;
	float x = 0.0f, y = 0.0f;
	uint32_t W = 0;
#pragma unroll 1
	for (int jj = 0; jj < 4; ++jj) {
		if constexpr (MODE == LSD_MODE_TILE) tile_raw8(m, xs, ys, dx, dy, xo, yo, x, y, W);
		else if constexpr (MODE == LSD_MODE_TILEC) tilec_raw8(m, xs, ys, dx, dy, xo, yo, x, y, W);
		else
#pragma unroll
		for (int j = 0; j < 8; ++j) {
			x = xo + xs; y = yo + ys;                   // x = x_offset + x_start
			if (MODE == LSD_MODE_TILE) W = __builtin_amdgcn_alignbit(tile_raw(m, x, y), W, 1);
			else W = __builtin_amdgcn_alignbit(win_raw<false>(m, (int)x, (int)y), W, 1);       // LSD_MODE_GLOBAL, no row cache
			xo += dx; yo += dy;                         // x_offset += dx
		}
	}
	Wm = W; n = 32u;
	if (!in_image(m, x, y)) {
		float rx = xo0, ry = yo0;
#pragma unroll 1
		for (n = 0; n < 32u; ++n) {
			if (!in_image(m, rx + xs, ry + ys)) break;
			rx += dx; ry += dy;
		}
	}
}

#define W_PAR_LANES 8u                 // lanes (= 32-sample batches walked at once) per long ray (2 / 4 lanes per ray for 16 / 32 rays: measured, no gain)
#ifndef W_PAR_MAX_RAYS
#define W_PAR_MAX_RAYS 8u              // more long rays than this in a unit: walk them batch after batch, one ray per lane
#endif

// The long rays of a unit, W_PAR_LANES lanes per ray: lane t of a group samples batch j0 + t of its ray (start offsets from
// the table Buffers::ray_off), then every lane of the group runs ray_batch's gap state machine over the group's batches
// in order.  `s`, `status`, `steps` of the lanes whose rays were walked are advanced exactly as W_PAR_LANES calls of
// ray_batch would have.  T <= 31.
template <int MODE>
__device__ __forceinline__ void long_rays_round(const Win &m, const float *ray_off, uint32_t u, float xs, float ys, float dx, float dy, uint32_t T,
                                                unsigned long long cont, RayState &s, int &status, uint32_t &steps) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t q = lane / W_PAR_LANES, t = lane % W_PAR_LANES;
	// the q-th continuing ray of the wave is this group's ray
	unsigned long long c = cont;
	for (uint32_t k = 0; k < q && c; ++k) c &= c - 1ull;
	const bool have = c != 0ull;
	const uint32_t src = have ? (uint32_t)__builtin_ctzll(c) : 0u;
	unsigned long long sel = 0ull;                              // the rays taken this round (uniform)
	{
		unsigned long long cc = cont;
		for (uint32_t k = 0; k < 64u / W_PAR_LANES && cc; ++k) { sel |= cc & (~cc + 1ull); cc &= cc - 1ull; }
	}
	// the ray's state, from its own lane
	const float rdx = __shfl(dx, (int)src), rdy = __shfl(dy, (int)src);
	const uint32_t rk0 = __shfl(s.k0, (int)src);
	uint32_t g = __shfl(s.g, (int)src);
	uint32_t jg = __shfl(s.gk0, (int)src) >> 5, gj = __shfl(s.gj, (int)src);
	const uint32_t j0 = rk0 >> 5, i = u * 64u + src;
	uint32_t Wm = 0, n = 0;
	if (have) {
		const float2 o = ((const float2 *)ray_off)[(size_t)i * (SMH_RAY_OFF_BATCHES + 1u) + min(j0 + t, SMH_RAY_OFF_BATCHES)];
		sample32<MODE>(m, xs, ys, rdx, rdy, o.x, o.y, Wm, n);
	}
	uint32_t Wt[W_PAR_LANES], nt[W_PAR_LANES];
#pragma unroll
	for (uint32_t k = 0; k < W_PAR_LANES; ++k) { Wt[k] = __shfl(Wm, (int)(q * W_PAR_LANES + k)); nt[k] = __shfl(n, (int)(q * W_PAR_LANES + k)); }
	// ---- ray_batch's gap state machine over the W_PAR_LANES batches, in order ----
	int st = RAY_CONTINUE;
	uint32_t rsteps = 0, nexit = 0, jx = 0;
#pragma unroll
	for (uint32_t k = 0; k < W_PAR_LANES; ++k) {
		if (st == RAY_CONTINUE) {
			const uint32_t j = j0 + k, k0 = j << 5;
			const uint32_t valid = nt[k] >= 32u ? 0xFFFFFFFFu : ((1u << nt[k]) - 1u);
			const uint32_t Wv = Wt[k] & valid, Z = ~Wt[k] & valid;
			const unsigned long long Z64 = ((unsigned long long)Z << g) | ((1ull << g) - 1ull);
			unsigned long long R = Z64;
			const uint32_t L = T + 1u;
			uint32_t hv = 1u;
			while (hv * 2u <= L) { R &= R >> hv; hv *= 2u; }
			if (L > hv) R &= R >> (L - hv);
			if (R) {
				const uint32_t p = (uint32_t)__builtin_ctzll(R);    // start of the fatal run (a run start, or 0 = carried in)
				if (p >= g) { jg = j; gj = p - g; }
				rsteps = k0 + (p + T - g) + 1u;
				st = RAY_ABORTED;
			} else if (nt[k] < 32u) {
				rsteps = k0 + nt[k]; nexit = nt[k]; jx = j;
				st = RAY_LEFT_IMAGE;
			} else {
				const uint32_t msb = 31u - (uint32_t)__builtin_clz(Wv);   // no abort in a full batch with T <= 31: at least one white sample
				g = 31u - msb;
				if (g) { jg = j; gj = msb + 1u; }
			}
		}
	}
	// ---- back to the rays' own lanes ----
	const bool mine = (sel >> lane) & 1ull;
	const uint32_t leader = (uint32_t)__popcll(sel & ((1ull << lane) - 1ull)) * W_PAR_LANES;
	const int r_st = __shfl(st, (int)leader);
	const uint32_t r_g = __shfl(g, (int)leader), r_jg = __shfl(jg, (int)leader), r_gj = __shfl(gj, (int)leader);
	const uint32_t r_steps = __shfl(rsteps, (int)leader), r_nexit = __shfl(nexit, (int)leader), r_jx = __shfl(jx, (int)leader);
	if (mine) {
		const uint32_t myi = u * 64u + lane;
		const float2 *tab = (const float2 *)ray_off + (size_t)myi * (SMH_RAY_OFF_BATCHES + 1u);
		status = r_st;
		s.g = r_g; s.gj = r_gj; s.gk0 = r_jg << 5;
		if (r_st == RAY_CONTINUE) {
			s.k0 += 32u * W_PAR_LANES;                              // (s.bxo / s.byo are stale from here on: only the table is used)
		} else {
			steps += r_steps;
			if (r_st == RAY_ABORTED) { const float2 o = tab[min(r_jg, SMH_RAY_OFF_BATCHES)]; s.gxo = o.x; s.gyo = o.y; }
			else { const float2 o = tab[min(r_jx, SMH_RAY_OFF_BATCHES)]; s.bxo = o.x; s.byo = o.y; s.k0 = r_jx << 5; s.nexit = r_nexit; }
		}
	}
}

// One 64-ray unit of a candidate by one wave (find_longest_line, vision-cpu/src/lib.rs:387-449): every ray is walked for
// two 32-sample batches, which yields the step K at which its final gap began; rays still alive after that are walked to
// their end on the spot.  Exact end points (a replay of the reference's additions) only for the rays that can matter.
// Returns true for the wave that completes the candidate's last unit (the candidate is then ready to retire).
#ifdef SMH_LSD_WDEBUG
#define UPROF(i) do { const unsigned long long _n = __builtin_amdgcn_s_memtime(); uprof[i] += _n - ulast; ulast = _n; } while (0)
#define UPROF_PARAM , unsigned long long *uprof
#else
#define UPROF(i)
#define UPROF_PARAM
#endif
// The rays of unit u of the candidate whose pixel is (px, py) and start point (xs, ys): per lane the ray's key (len^2 bits << 32
// | ray index; 0 = not evaluated exactly: it cannot matter), its end point and the mask samples it took (added to `steps`).
__device__ __forceinline__ RayDir unit_dirs(uint32_t u) { return g_ray_table[min(u * 64u + (threadIdx.x & 63u), (uint32_t)SMH_LSD_RAYS - 1u)]; }
// (d = unit_dirs(u): a global load the caller may issue early; tag: where the window lies when cand_setup was given one; LEAN: the
// first batches through the search service's sampler, ray_batch)
template <int MODE, int G = 8, bool TAGGED = false, bool LEAN = false>
__device__ __forceinline__ void unit_rays(const Win &m, const uint32_t *wwin, const float *ray_off, uint32_t px, uint32_t py, float xs, float ys, uint32_t u, const RayDir d, float max_gap,
                                          unsigned long long &key, float &xe, float &ye, uint32_t &steps UPROF_PARAM, const WinTag *tag = nullptr) {
#ifdef SMH_LSD_WDEBUG
	unsigned long long ulast = __builtin_amdgcn_s_memtime();
#endif
	const uint32_t lane = threadIdx.x & 63u;
	const bool fast_gap = max_gap > 0.0f && max_gap <= 60000.0f;
	const uint32_t T = fast_gap ? (uint32_t)ceilf(max_gap) : 0u;
	const bool fast = fast_gap && in_image(m, xs, ys);
	const uint32_t i = u * 64u + lane;
	const bool valid = i < SMH_LSD_RAYS;
	const float dx = __uint_as_float(d.dx), dy = __uint_as_float(d.dy);
	xe = xs; ye = ys;
	uint32_t K = 0;
	int status = RAY_ABORTED;                                   // invalid lanes: "finished", K = 0
	bool exact = false;
	RayState s = {0.0f, 0.0f, 0u, 0u, 0.0f, 0.0f, 0u, 0u, 0u};
	if (valid) {
		if (fast) {
			// the first batches out of the candidate's window (the start point is in the image, within 2.5 px of the pixel)
			Win mw = m;
			mw.w2 = TAGGED ? window_base_at(wwin, tag->x0w, tag->y0) : window_base(wwin, px, py);
			status = RAY_CONTINUE;
#pragma unroll 1
			for (uint32_t bi = 0; bi < W_A_BATCHES && status == RAY_CONTINUE; ++bi) status = ray_batch<LSD_MODE_WIN2, G, LEAN>(mw, xs, ys, dx, dy, T, s, steps);
			if (status == RAY_ABORTED) K = s.gk0 + s.gj;
		} else {
			cast_ray_literal(m, xs, ys, max_gap, dx, dy, xe, ye, steps);
			exact = true;
		}
	}
	const bool was_long = status == RAY_CONTINUE;               // a long ray (runs along a marker line): to its end, exactly
	unsigned long long cont = __ballot(was_long);
	UPROF(8);
	if (cont) {
		const bool par = ray_off != nullptr && fast && T <= 31u;
		// many long rays: one per lane, batch after batch; few: W_PAR_LANES batches of a ray at once (the tail of the longest
		// rays would otherwise be walked 32 samples at a time by a wave with one or two active lanes)
		while (cont && (!par || (uint32_t)__popcll(cont) > W_PAR_MAX_RAYS)) {
			if (status == RAY_CONTINUE) status = ray_batch<MODE>(m, xs, ys, dx, dy, T, s, steps);
			cont = __ballot(status == RAY_CONTINUE);
		}
		while (cont) {
			// (a ray longer than the offset table reaches cannot occur for a supported frame size; it would be walked serially)
			const bool fits = __all(status != RAY_CONTINUE || (s.k0 >> 5) + W_PAR_LANES <= SMH_RAY_OFF_BATCHES);
			if (!fits) {
				if (status == RAY_CONTINUE) {
					const float2 o = ((const float2 *)ray_off)[(size_t)i * (SMH_RAY_OFF_BATCHES + 1u) + min(s.k0 >> 5, SMH_RAY_OFF_BATCHES)];
					s.bxo = o.x; s.byo = o.y;
					status = ray_batch<MODE>(m, xs, ys, dx, dy, T, s, steps);
				}
			}
			else long_rays_round<MODE>(m, ray_off, u, xs, ys, dx, dy, T, cont, s, status, steps);
			cont = __ballot(status == RAY_CONTINUE);
		}
	}
	UPROF(9);
	if (was_long) {
		ray_endpoint(m, status, s, xs, ys, dx, dy, xe, ye);
		exact = true;
	} else if (valid && !exact && (status == RAY_LEFT_IMAGE || K > SMH_LSD_REJECT_K)) {
		// left the image (may end with length 0), or its gap starts at step >= 50: a ray that can be the longest of an
		// ACCEPTABLE candidate.  A ray whose gap starts at step K <= 49 is shorter than 50 px (it ends K - 1 unit steps from
		// the start, +-0.25): it never wins in a candidate find_lines keeps (len^2 > 2500, lsd.rs:94), and in one it rejects
		// nobody asks which ray was the longest -- so its end point is never needed.
		ray_endpoint(m, status, s, xs, ys, dx, dy, xe, ye);
		exact = true;
	}
	UPROF(10);
	key = 0ull;
	if (valid && exact) {
		const float ddx = xs - xe, ddy = ys - ye;               // p0.distance_sqr(&p1)
		key = ((unsigned long long)__float_as_uint(ddx * ddx + ddy * ddy) << 32) | i;
	}
}

template <int MODE>
__device__ bool unit_cast(const Win &m, const uint32_t *wwin, const float *ray_off, WSlot &sl, uint32_t *win_free, uint32_t u, float max_gap UPROF_PARAM) {
	const uint32_t lane = threadIdx.x & 63u;
	unsigned long long key;
	float xe, ye;
	uint32_t steps = 0;
#ifdef SMH_LSD_WDEBUG
	unit_rays<MODE>(m, wwin, ray_off, sl.px, sl.py, sl.ptx, sl.pty, u, unit_dirs(u), max_gap, key, xe, ye, steps, uprof);
	unsigned long long ulast = __builtin_amdgcn_s_memtime();
#else
	unit_rays<MODE>(m, wwin, ray_off, sl.px, sl.py, sl.ptx, sl.pty, u, unit_dirs(u), max_gap, key, xe, ye, steps);
#endif
	slot_merge_best(sl, key, xe, ye);
	const uint32_t wsteps = wave_sum32_dpp(steps);
	uint32_t prev = 0;
	if (lane == 0) {
		__hip_atomic_fetch_add(&sl.steps, wsteps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		prev = __hip_atomic_fetch_sub(&sl.pending, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
	}
	UPROF(11);
	if (uniform_u32(prev) == 1u) {                              // the candidate's last unit: ready to retire
#ifdef SMH_LSD_WDEBUG
		if (lane == 0) sl.t_done = __builtin_amdgcn_s_memtime();
#endif
		// every unit has been cast: nobody reads the candidate's window any more -- it goes back NOW, not when the candidate
		// retires (in order, possibly behind a slow one): the windows bound the candidates being CAST, the reorder buffer the
		// ones waiting for their turn
		if (lane == 0) __hip_atomic_fetch_or(win_free, 1u << sl.win, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
		if (lane == 0) W_ST_REL(&sl.state, (uint32_t)W_DONE);
		return true;
	}
	return false;
}

// The oldest candidate with a unit nobody has taken yet: lane k looks at the k-th slot behind the head.  -> slot, unit.
__device__ __forceinline__ bool claim_unit(WShared &ws, uint32_t &slot, uint32_t &unit) {
	const uint32_t lane = threadIdx.x & 63u;
	while (true) {
		const uint32_t head = W_LD(&ws.head), tail = W_LD_ACQ(&ws.tail);
		unsigned long long td = 0ull;
		const uint32_t s = (head + lane) % W_ROB;
		if (lane < tail - head && lane < W_ROB) td = __hip_atomic_load(&ws.rob[s].todo, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
		const unsigned long long any = __ballot(td != 0ull);
		if (!any) return false;
		const uint32_t src = (uint32_t)__builtin_ctzll(any);
		const uint32_t sidx = (uniform_u32(head) + src) % W_ROB;
		unsigned long long got = 0ull;
		if (lane == 0) {
			unsigned long long cur = __hip_atomic_load(&ws.rob[sidx].todo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
			while (cur) {
				const unsigned long long bit = cur & (~cur + 1ull);
				if (__hip_atomic_compare_exchange_strong(&ws.rob[sidx].todo, &cur, cur & ~bit, __ATOMIC_ACQUIRE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) { got = bit; break; }
			}
		}
		const uint32_t glo = uniform_u32((uint32_t)got), ghi = uniform_u32((uint32_t)(got >> 32));
		if (glo | ghi) {
			slot = sidx;
			unit = glo ? (uint32_t)__builtin_ctz(glo) : 32u + (uint32_t)__builtin_ctz(ghi);
			return true;
		}
		// somebody else took the last unit of that candidate meanwhile: look again
	}
}

// 8-byte granules of the helper exchange (smh_kernels.h, FarmEntry): agent-scope relaxed atomics = `global_* ... sc1`
__device__ __forceinline__ void g_st64(unsigned long long *p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long g_ld64(const unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long farm_post_word(uint32_t epoch, uint32_t k, uint32_t px, uint32_t py) {
	return ((unsigned long long)(epoch & 0xFFFFu) << 48) | ((unsigned long long)((k + 1u) & 0xFFFFFFu) << 24) | ((unsigned long long)(py & 0xFFFu) << 12) | (px & 0xFFFu);
}
__device__ __forceinline__ uint32_t farm_done_tag(uint32_t epoch, uint32_t k) { return ((epoch & 0xFFFFu) << 16) | ((k + 1u) & 0xFFFFu); }
// One wave, holding the lock: retire finished candidates in dispatch order (lsd.rs:84-104 for each).
#define LATE_MIN_LEFT 16u               // list entries a frame must have left for a helper to bother
template <int MODE>
__device__ __forceinline__ void wave_retire(const Win &m, WShared &ws, FarmFrame *farm, uint32_t b_epoch) {
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t head = W_LD(&ws.head);
	const uint32_t tail = W_LD(&ws.tail);
	uint32_t spec = ws.spec;
	const uint32_t spec_max = W_SPEC_MAX + (W_LD(&ws.farm_on) ? SMH_FARM_RING : 0u);
	while (head != tail) {
		WSlot &sl = ws.rob[head % W_ROB];
		uint32_t st = W_LD_ACQ(&sl.state);
		if (st == W_REMOTE) {                                   // cast by the helper workgroup: has its result arrived?
			FarmEntry *e = &farm->ring[sl.win];
			const unsigned long long dn = g_ld64(&e->done);
			if ((dn >> 32) != sl.tag) break;
			// (the helper drained its payload stores before it stored `done`: sc1 loads see them)
			const unsigned long long bw = g_ld64(&e->best), ew = g_ld64(&e->end), sw = g_ld64(&e->start);
			if (lane == 0) {
				sl.best = bw; sl.ex = __uint_as_float((uint32_t)ew); sl.ey = __uint_as_float((uint32_t)(ew >> 32));
				sl.ptx = __uint_as_float((uint32_t)sw); sl.pty = __uint_as_float((uint32_t)(sw >> 32));
				sl.steps = (uint32_t)dn;
				W_ST(&ws.farm_retired, ws.farm_retired + 1u);
				W_ST(&sl.state, (uint32_t)W_DONE);
			}
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
			st = W_DONE;
		}                                                       // (a local candidate gave its window back when its last unit was merged)
		if (st != W_DONE) break;
		bool accepted = false;
		uint32_t n_lines = W_LD(&ws.n_lines);
		if (!W_LD(&ws.frame_done)) {
			const float cx = (float)sl.px, cy = (float)sl.py;
			bool skip = false;                                   // a line accepted after the dispatch: the scan would not have visited it
			for (uint32_t l = sl.lines_seen; l < n_lines; ++l) skip = skip || near_line(cx, cy, ws.lines[l][0], ws.lines[l][1], ws.lines[l][2], ws.lines[l][3]);
			if (skip) WDBG(2, 1u);
			if (!skip) {
				const float len = __uint_as_float((uint32_t)(sl.best >> 32));
				float ex = 0.0f, ey = 0.0f;
				const bool accept = len > SMH_LSD_ACCEPT_LEN_SQ;
				accepted = accept;
				if (accept) get_centre(m, sl.ex, sl.ey, ex, ey);
#ifdef SMH_LSD_WDEBUG
				if (lane == 0) {
					const unsigned long long now = __builtin_amdgcn_s_memtime(), dtl = now - sl.t_disp;
					ws.lat[accept ? 0 : 2] += dtl; ws.lat[accept ? 1 : 3] += 1ull;
					if (sl.t_setup >= sl.t_disp && sl.t_done >= sl.t_setup) { ws.lat[4] += sl.t_setup - sl.t_disp; ws.lat[5] += sl.t_done - sl.t_setup; ws.lat[6] += now - sl.t_done; ws.lat[7] += 1ull; }
				}
#endif
				if (lane == 0) {
					ws.rounds += 1u;
					ws.steps += sl.steps;
					if (accept) {
						ws.lines[n_lines][0] = sl.ptx; ws.lines[n_lines][1] = sl.pty; ws.lines[n_lines][2] = ex; ws.lines[n_lines][3] = ey;
						const ProxLine pl = prox_line(sl.ptx, sl.pty, ex, ey);
						ws.prox_a[n_lines] = pl.a; ws.prox_d[n_lines][0] = pl.dxl; ws.prox_d[n_lines][1] = pl.dyl;
						W_ST_REL(&ws.n_lines, n_lines + 1u);
						if (n_lines + 1u == SMH_LSD_MAX_LINES) W_ST(&ws.frame_done, 1u);
					}
				}
			}
		}
		if (lane == 0) W_ST(&sl.state, (uint32_t)W_FREE);
		++head;
		// Speculation width: candidates dispatched before a line was accepted mostly lie next to it and are dropped when
		// they retire (wasted casts), and acceptances cluster (the first pixels of a marker): few candidates in flight
		// right after an acceptance, twice as many after every candidate retired without one.
		spec = accepted ? W_SPEC_MIN : min(W_SPEC_GROW(spec), spec_max);  // (one window / one ring entry per candidate in flight)
	}
	if (lane == 0) { W_ST(&ws.head, head); W_ST(&ws.spec, spec); }
	if (farm && ws.late && !W_LD(&ws.farm_on)) {
		// late helpers: a frame still at work LATE_WANT_CYCLES after it began says so, with the list entries it has yet to visit
		// (what a finished workgroup picks its frame by), refreshed every 16 stays under the lock; 1074 x 1024 cycles by default:
		// a mean frame of the synthetic workload takes 1.04 M
		const uint32_t tick = W_LD(&ws.want_tick);
		const bool set = W_LD(&ws.want_set) != 0u;
		const bool due = set ? (tick & 15u) == 15u : __builtin_amdgcn_s_memtime() - ws.t0 > ws.late_cycles;
		if (lane == 0) {
			if (set) W_ST(&ws.want_tick, tick + 1u);
			if (due) {
				const uint32_t left = ws.disp_end - min(W_LD(&ws.disp_e), ws.disp_end);
				g_st64(&farm->want, ((unsigned long long)(b_epoch & 0xFFFFu) << 48) | left);
				W_ST(&ws.want_set, 1u);
			}
		}
	}
}

// One wave, holding the lock: the next surviving white pixel in raster order -> (px, py), or false when the chunk has
// none left.  Survivor words are brought up to date with the accepted lines as the scan reaches them.
__device__ __forceinline__ bool wave_dispatch(WShared &ws, const uint32_t *list, uint32_t *survw, uint32_t wy0, uint32_t wwords, int xorg, uint32_t &px, uint32_t &py) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t n_lines = W_LD(&ws.n_lines), end = ws.disp_end;
	// The 64 entries a pass looks at are an ALIGNED chunk of the list, not the 64 behind the cursor: an entry is brought up to
	// date with every accepted line the first time a pass covers it, one lane per entry -- with a window that slides with the
	// cursor that was one new entry per dispatch, i.e. the whole loop over the lines (24 of them on a busy screenshot) for a
	// single lane, under the lock, every time; with chunks it is 64 entries at once, once per chunk and per new line.
	const uint32_t first = W_LD(&ws.disp_e);
	uint32_t e0 = first & ~63u;
	while (e0 < end) {
		const uint32_t e = e0 + lane;
		uint32_t w = 0;
		float fpx0 = 0.0f, fpy = 0.0f;
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
#ifdef SMH_LSD_WDEBUG
				atomicAdd(&ws.dbg[5], 1u); if (!w) atomicAdd(&ws.dbg[6], 1u);
#endif
				survw[e] = w;
				ws.stag[e] = (unsigned char)n_lines;
			}
		}
		const unsigned long long any = __ballot(w != 0u);
		WDBG(3, 1u);
		if (any) {
			const uint32_t src = (uint32_t)__builtin_ctzll(any);
			const uint32_t ww = (uint32_t)__builtin_amdgcn_readlane((int)w, (int)src);
			const uint32_t bit = (uint32_t)__builtin_ctz(ww);
			px = (uint32_t)((int)bcast_f(fpx0, src) + (int)bit);
			py = (uint32_t)bcast_f(fpy, src);
			if (lane == 0) survw[e0 + src] = ww & (ww - 1u);
			if (lane == 0) W_ST(&ws.disp_e, e0 + src + ((ww & (ww - 1u)) ? 0u : 1u));
			return true;
		}
		e0 += 64u;
	}
	if (lane == 0) W_ST(&ws.disp_e, end);
	return false;
}

// LSD_MODE_TILE: words of LDS the mask of a frame takes -- (tile_cap + 1) tiles of 8 words, then the 16-bit index
__host__ __device__ inline uint32_t tile_idx_pitch(uint32_t rw) { return ((rw + 31u) >> 5) + 4u; }
__host__ __device__ inline uint32_t tile_idx_words(uint32_t rw, uint32_t rh) { return ((((rh + 7u) >> 3) + 2u) * tile_idx_pitch(rw) + 1u) / 2u; }
__host__ __device__ inline uint32_t tile_mask_words(uint32_t rw, uint32_t rh, uint32_t tile_cap) { return (tile_cap + 1u) * 8u + tile_idx_words(rw, rh); }
// list entries per segment: a 1080p scene has 300-700 non-zero mask words, a 1440p scene up to 1200
inline uint32_t tile_list_cap_for(const Geom &g) { return g.rh > 900u ? W_LIST_CAP_MAX : W_LIST_CAP_MAX / 2u; }
// Tiles a workgroup has room for: the dynamic LDS (tile store + candidate lists) stays within 60 KB, so that with the
// kernel's 17 KB of static LDS two workgroups share a CU.  1023 tiles at 1080p / 1440p (a scene uses 40-260), 541 at 4K.
// A frame whose index alone leaves no room for 256 tiles in that (8K: 106 KB of index) gets 140 KB, one workgroup per CU.
#define LSD_TILE_DYN_LDS_2PER_CU 61440u
#define LSD_TILE_DYN_LDS_MAX 143360u
inline uint32_t tile_cap_for(const Geom &g) {
	const uint32_t idx = tile_idx_words(g.rw, g.rh);
	for (uint32_t budget : {LSD_TILE_DYN_LDS_2PER_CU, LSD_TILE_DYN_LDS_MAX}) {
		const uint32_t words = budget / 4u - 2u * tile_list_cap_for(g) - W_NWIN * W_WIN_STRIDE;
		const uint32_t cap = words > idx + 16u ? (words - idx) / 8u - 1u : 0u;
		if (cap >= 256u || budget == LSD_TILE_DYN_LDS_MAX) return std::min<uint32_t>(std::max<uint32_t>(cap, 1u), 1023u);
	}
	return 1u;
}

// Build the tile store of frame f in `smem` (tile_mask_words words).  -> false when the frame has more than tile_cap
// non-empty tiles (it is then left to the fallback kernel).  Tile numbers depend on the order the threads get there;
// nothing observable does.
// WAVE: the builder is ONE wave of a workgroup whose waves work on different frames (k_lsd_service): its lanes are the
// "threads", and the barriers are the wave's own.
template <bool WAVE>
__device__ __forceinline__ void team_barrier() {
	if (WAVE) { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); }
	else __syncthreads();
}
template <bool WAVE = false>
__device__ __forceinline__ bool frame_setup_tile(const Geom &g, const Buffers &b, uint32_t f, const FrameAux &aux, uint32_t *smem, uint32_t tile_cap, uint32_t *ntiles, FrameView &v) {
	const uint32_t tid = WAVE ? (threadIdx.x & 63u) : threadIdx.x, bs = WAVE ? 64u : blockDim.x;
	const uint32_t *gbits = b.bits + (size_t)f * g.bits_stride_w;
	const uint32_t TW = (g.rw + 31u) >> 5, TWP = tile_idx_pitch(g.rw), gp = g.bits_pitch_w;
	uint32_t *tiles = smem;
	uint32_t *idxw = smem + (tile_cap + 1u) * 8u;
	const uint32_t idx_words = tile_idx_words(g.rw, g.rh);
	for (uint32_t i = tid; i < idx_words; i += bs) idxw[i] = 0u;
	if (tid < 8u) tiles[tid] = 0u;
	if (tid == 0) *ntiles = 0u;
	team_barrier<WAVE>();
	LdsU16 *idx = (LdsU16 *)idxw;
	const uint32_t ty0 = aux.y_min >> 3, nty = (aux.y_max >> 3) - ty0 + 1u;
	// tile columns that can hold a set bit (the box is in words of the global rows, which start m_xoff bits left of pixel 0)
	const uint32_t tx0 = aux.w_min ? aux.w_min - 1u : 0u, tx1 = min(aux.w_max, TW - 1u), ntx = tx1 >= tx0 ? tx1 - tx0 + 1u : 0u;
	for (uint32_t t = tid; t < nty * ntx; t += bs) {
		const uint32_t ty = ty0 + t / ntx, tx = tx0 + t % ntx;
		uint32_t wv[8], any = 0u;
#pragma unroll
		for (uint32_t r = 0; r < 8u; ++r) {
			const uint32_t y = ty * 8u + r;
			uint32_t val = 0u;
			if (y >= aux.y_min && y <= aux.y_max && tx < gp) {
				const uint32_t *src = gbits + (size_t)y * gp + tx;
				const uint32_t lo = src[0], hi = (tx + 1u < gp) ? src[1] : 0u;
				val = __builtin_amdgcn_alignbit(hi, lo, g.m_xoff);       // bit x of the row = pixel x
			}
			wv[r] = val; any |= val;
		}
		if (any) {
			const uint32_t slot = atomicAdd(ntiles, 1u);
			if (slot < tile_cap) {
#pragma unroll
				for (uint32_t r = 0; r < 8u; ++r) tiles[(slot + 1u) * 8u + r] = wv[r];
				idx[(ty + 1u) * TWP + tx + 2u] = (unsigned short)(slot + 1u);
			}
		}
	}
	team_barrier<WAVE>();
	Win &m = v.m;
	v.gbits = gbits;
	m.w = g.rw; m.h = g.rh; m.wf = (float)g.rw; m.hf = (float)g.rh;
	m.p = smem; m.pitch4 = 0u; m.y_lo = 0; m.xbias = 0; m.rows_hi = 0u; m.cols_hi = 0u;
	m.rows0 = nullptr; m.ylo_f = 0.0f; m.yhi_f = 0.0f;
	m.c_p = (const LdsWord *)smem; m.c_y0 = 0u; m.c_rows = 0u; m.c_pitch4 = 0u;
	m.t_idx = (const LdsU16 *)idx + TWP + 2u; m.t_tiles = (const LdsWord *)tiles; m.t_pitch = TWP; m.tiled = true;
	m.tc_rows = nullptr; m.tc_groups = 0u; m.compact = false;
	v.wy0 = aux.y_min; v.wrows = aux.y_max - aux.y_min + 1u; v.wwords = TW; v.xorg = 0;
	v.c_pitch = 0u; v.c_cap_rows = 0u;
	return *ntiles <= tile_cap;
}

// ---- the same store from the pass's tile-major mask (smh_kernels.h, "the mask as the streaming passes leave it") ------------------
// ONE wave (the search service).  The occupancy bytes of the bounding box's tile rows name the non-empty tiles of the bit rows'
// word columns (one coalesced load); their coordinates are spread over the lanes through `tmp` (words of the wave's own LDS
// block where the lists and the window will live: nothing is there between frames); then every lane fetches one tile -- 32
// contiguous bytes, two chunks of 64 tiles in flight -- and files it: the bit rows start m_xoff bits left of pixel 0, so a
// word column's tile feeds the search's tile of the same column (its bits >> m_xoff) and the high end of the one to its left
// (its low m_xoff bits).  Within one such phase the lanes' targets are distinct (the fetched tiles are), phases are separated
// by wave barriers, so a tile is allocated once (ballot + prefix count) and OR-ed into afterwards without atomics.
// -> 0 built; 1 more than tile_cap tiles (the frame is left to the scan on the mask in global memory); 2 more non-empty tiles
//    than `tmp` holds: the caller walks the bit rows (frame_setup_tile)
__device__ __forceinline__ uint32_t wave_excl_prefix32(uint32_t v, uint32_t lane, uint32_t *total) {
	uint32_t incl = v;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o); if (lane >= (uint32_t)o) incl += t; }
	*total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
	return incl - v;
}
// The non-empty tiles of the bit rows' word columns, from the occupancy bytes of the bounding box's tile rows (a dword = four waves
// of the pass = 32 tiles; one coalesced load, four dwords per lane in flight): their coordinates (ty << 16 | wx) into tmp[0 .. n), in
// raster order (a prefix sum over the lanes' popcounts).  -> n (may exceed tmp_words: then only the first tmp_words were stored)
__device__ __forceinline__ uint32_t occ_tile_list(const Geom &g, const Buffers &b, uint32_t f, const FrameAux &aux, uint32_t *tmp, uint32_t tmp_words) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t ty0 = aux.y_min >> 3, nty = (aux.y_max >> 3) - ty0 + 1u;
	const uint32_t opitch = occ_pitch(g), dpr = opitch >> 2, items = nty * dpr;
	const uint32_t *occ32 = (const uint32_t *)(b.occ + (size_t)f * occ_stride(g) + (size_t)ty0 * opitch);
	uint32_t n_g = 0;                                           // (uniform)
	for (uint32_t base = 0; base < items; base += 256u) {
		uint32_t d[4];
#pragma unroll
		for (uint32_t k = 0; k < 4u; ++k) { const uint32_t i = base + k * 64u + lane; d[k] = i < items ? occ32[i] : 0u; }
#pragma unroll
		for (uint32_t k = 0; k < 4u; ++k) {
			if (base + k * 64u >= items) break;
			const uint32_t i = base + k * 64u + lane;
			uint32_t total;
			uint32_t off = n_g + wave_excl_prefix32((uint32_t)__builtin_popcount(d[k]), lane, &total);
			const uint32_t row = i / dpr, ty = ty0 + row, wb = (i - row * dpr) * 32u;
			for (uint32_t dd = d[k]; dd; dd &= dd - 1u) {
				if (off < tmp_words) tmp[off] = (ty << 16) | (wb + (uint32_t)__builtin_ctz(dd));
				++off;
			}
			n_g += total;
		}
	}
	team_barrier<true>();
	return n_g;
}
__device__ __forceinline__ uint32_t frame_setup_tile_occ(const Geom &g, const Buffers &b, uint32_t f, const FrameAux &aux, uint32_t *smem, uint32_t tile_cap, uint32_t *ntiles, FrameView &v,
                                                         uint32_t *tmp, uint32_t tmp_words) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t TW = (g.rw + 31u) >> 5, TWP = tile_idx_pitch(g.rw), gp = g.bits_pitch_w, xoff = g.m_xoff;
	uint32_t *tiles = smem;
	uint32_t *idxw = smem + (tile_cap + 1u) * 8u;
	const uint32_t idx_words = tile_idx_words(g.rw, g.rh);
	for (uint32_t i = lane; i < idx_words; i += 64u) idxw[i] = 0u;
	if (lane < 8u) tiles[lane] = 0u;
	// ---- which tiles ----
	const uint32_t n_g = occ_tile_list(g, b, f, aux, tmp, tmp_words);
	if (n_g > tmp_words) return 2u;
	// ---- fetch and file them ----
	const uint32_t *tg = b.tiled + (size_t)f * tiled_stride_w(g);
	LdsU16 *idx = (LdsU16 *)idxw;
	uint32_t count = 0;                                         // tiles of the store so far (uniform)
	auto place = [&](uint32_t tx, uint32_t ty, bool any, const uint32_t (&w)[8]) {
		LdsU16 *ip = idx + (any ? (ty + 1u) * TWP + tx + 2u : 0u);
		uint32_t slot = any ? (uint32_t)*ip : 0u;
		const bool fresh = any && slot == 0u;
		const unsigned long long bal = __ballot(fresh);
		if (fresh) {
			slot = count + (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u)) + 1u;
			if (slot <= tile_cap) *ip = (unsigned short)slot;
		}
		count += (uint32_t)__popcll(bal);
		if (any && slot <= tile_cap) {
			uint32_t *t = tiles + slot * 8u;
			if (fresh) {
#pragma unroll
				for (uint32_t r = 0; r < 8u; ++r) t[r] = w[r];
			} else {
#pragma unroll
				for (uint32_t r = 0; r < 8u; ++r) t[r] |= w[r];
			}
		}
		team_barrier<true>();
	};
	auto file_tile = [&](bool valid, uint32_t c, const uint4 &lo, const uint4 &hi) {
		const uint32_t ty = c >> 16, wx = c & 0xFFFFu;
		uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
		for (uint32_t r = 0; r < 8u; ++r) if (ty * 8u + r >= g.rh) w[r] = 0u;     // (the last tile row's rows beyond the image are never written)
		uint32_t m[8], any = 0u;
#pragma unroll
		for (uint32_t r = 0; r < 8u; ++r) { m[r] = w[r] >> xoff; any |= m[r]; }
		place(wx, ty, valid && wx < TW && any != 0u, m);
		if (xoff) {                                             // (uniform)
			any = 0u;
#pragma unroll
			for (uint32_t r = 0; r < 8u; ++r) { m[r] = w[r] << (32u - xoff); any |= m[r]; }
			place(wx - 1u, ty, valid && wx >= 1u && wx - 1u < TW && any != 0u, m);
		}
	};
	for (uint32_t e0 = 0; e0 < n_g; e0 += 128u) {
		const uint32_t eA = e0 + lane, eB = eA + 64u;
		uint32_t cA = 0u, cB = 0u;
		uint4 a0 = {0u, 0u, 0u, 0u}, a1 = a0, b0 = a0, b1 = a0;
		if (eA < n_g) { cA = tmp[eA]; const uint4 *src = (const uint4 *)(tg + ((size_t)(cA >> 16) * gp + (cA & 0xFFFFu)) * 8u); a0 = src[0]; a1 = src[1]; }
		if (eB < n_g) { cB = tmp[eB]; const uint4 *src = (const uint4 *)(tg + ((size_t)(cB >> 16) * gp + (cB & 0xFFFFu)) * 8u); b0 = src[0]; b1 = src[1]; }
		file_tile(eA < n_g, cA, a0, a1);
		if (e0 + 64u < n_g) file_tile(eB < n_g, cB, b0, b1);
	}
	if (lane == 0) *ntiles = count;
	team_barrier<true>();
	Win &m = v.m;
	v.gbits = b.bits + (size_t)f * g.bits_stride_w;
	m.w = g.rw; m.h = g.rh; m.wf = (float)g.rw; m.hf = (float)g.rh;
	m.p = smem; m.pitch4 = 0u; m.y_lo = 0; m.xbias = 0; m.rows_hi = 0u; m.cols_hi = 0u;
	m.rows0 = nullptr; m.ylo_f = 0.0f; m.yhi_f = 0.0f;
	m.c_p = (const LdsWord *)smem; m.c_y0 = 0u; m.c_rows = 0u; m.c_pitch4 = 0u;
	m.t_idx = (const LdsU16 *)idx + TWP + 2u; m.t_tiles = (const LdsWord *)tiles; m.t_pitch = TWP; m.tiled = true;
	m.tc_rows = nullptr; m.tc_groups = 0u; m.compact = false;
	v.wy0 = aux.y_min; v.wrows = aux.y_max - aux.y_min + 1u; v.wwords = TW; v.xorg = 0;
	v.c_pitch = 0u; v.c_cap_rows = 0u;
	return count <= tile_cap ? 0u : 1u;
}

// ---- LSD_MODE_TILEC: the tile store behind the compact index (Win::tc_rows; the search service above 1080p) -----------------
__host__ __device__ inline uint32_t tilec_groups(uint32_t rw) { return (tile_idx_pitch(rw) + 63u) >> 6; }
__host__ __device__ inline uint32_t tilec_idx_words(uint32_t rw, uint32_t rh) { return (((rh + 7u) >> 3) + 2u) * tilec_groups(rw) * 4u; }
__host__ __device__ inline uint32_t tilec_mask_words(uint32_t rw, uint32_t rh, uint32_t tile_cap) { return (tile_cap + 1u) * 8u + tilec_idx_words(rw, rh); }
// Built by ONE wave, tile row by tile row (two at a time where a row's tile columns fit half a wave), so that the non-empty tiles
// are numbered in raster order as the index wants them: the wave's ballot IS the row's occupancy mask, no atomics on a counter.
// -> false when the frame has more than tile_cap non-empty tiles (left to the scan on the mask in global memory).
__device__ __forceinline__ bool frame_setup_tilec(const Geom &g, const Buffers &b, uint32_t f, const FrameAux &aux, uint32_t *smem, uint32_t tile_cap, uint32_t *ntiles, FrameView &v) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t *gbits = b.bits + (size_t)f * g.bits_stride_w;
	const uint32_t TW = (g.rw + 31u) >> 5, TWP = tile_idx_pitch(g.rw), gp = g.bits_pitch_w, G = tilec_groups(g.rw);
	uint32_t *tiles = smem;
	uint32_t *idxw = smem + (tile_cap + 1u) * 8u;
	const uint32_t idx_words = tilec_idx_words(g.rw, g.rh);
	for (uint32_t i = lane; i < idx_words; i += 64u) idxw[i] = 0u;
	if (lane < 8u) tiles[lane] = 0u;
	team_barrier<true>();
	uint32_t *rows0 = idxw + G * 4u;                            // the entry of (tile row 0, group 0)
	const uint32_t ty0 = aux.y_min >> 3, nty = (aux.y_max >> 3) - ty0 + 1u;
	const uint32_t tx0 = aux.w_min ? aux.w_min - 1u : 0u, tx1 = min(aux.w_max, TW - 1u), ntx = tx1 >= tx0 ? tx1 - tx0 + 1u : 0u;
	const bool two = ntx <= 32u;
	const uint32_t sub = two ? lane >> 5 : 0u, k = two ? lane & 31u : lane, step = two ? 2u : 1u;
	uint32_t count = 0;                                         // non-empty tiles so far (uniform)
	// (a bounding box more than 64 tile columns wide -- ROIs beyond 2048 px: 5120 x 1440 -- : a tile row in chunks of 64 columns.
	// Round 5's builder looked at the first 64 columns only; the round-6 fuzz over that frame size found it.)
	for (uint32_t r = 0; r < nty && ntx > 64u; ++r) {
		const uint32_t ty = ty0 + r;
		uint32_t row_count = 0;
		for (uint32_t c0 = 0; c0 < ntx; c0 += 64u) {
			const uint32_t tx = tx0 + c0 + lane;
			const bool active = c0 + lane < ntx;
			uint32_t wv[8], any = 0u;
#pragma unroll
			for (uint32_t q = 0; q < 8u; ++q) {
				const uint32_t y = ty * 8u + q;
				uint32_t val = 0u;
				if (active && y >= aux.y_min && y <= aux.y_max && tx < gp) {
					const uint32_t *src = gbits + (size_t)y * gp + tx;
					const uint32_t lo = src[0], hi = (tx + 1u < gp) ? src[1] : 0u;
					val = __builtin_amdgcn_alignbit(hi, lo, g.m_xoff);   // bit x of the row = pixel x
				}
				wv[q] = val; any |= val;
			}
			const unsigned long long bal = __ballot(active && any != 0u);
			const uint32_t slot = count + row_count + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
			if (active && any != 0u) {
				if (slot < tile_cap) {
#pragma unroll
					for (uint32_t q = 0; q < 8u; ++q) tiles[(slot + 1u) * 8u + q] = wv[q];
				}
				const uint32_t col = tx + 2u;
				atomicOr(rows0 + (ty * G + (col >> 6)) * 4u + ((col & 63u) >> 5), 1u << (col & 31u));
			}
			row_count += (uint32_t)__popcll(bal);
		}
		team_barrier<true>();
		if (lane < G) {
			uint32_t *row = rows0 + ty * G * 4u;
			uint32_t base = count;
			for (uint32_t h = 0; h < lane; ++h) base += (uint32_t)__builtin_popcount(row[h * 4u]) + (uint32_t)__builtin_popcount(row[h * 4u + 1u]);
			row[lane * 4u + 2u] = base;
		}
		count += row_count;
	}
	for (uint32_t r = 0; r < nty && ntx != 0u && ntx <= 64u; r += step) {
		const uint32_t ty = ty0 + r + sub, tx = tx0 + k;
		const bool active = k < ntx && r + sub < nty;
		uint32_t wv[8], any = 0u;
#pragma unroll
		for (uint32_t q = 0; q < 8u; ++q) {
			const uint32_t y = ty * 8u + q;
			uint32_t val = 0u;
			if (active && y >= aux.y_min && y <= aux.y_max && tx < gp) {
				const uint32_t *src = gbits + (size_t)y * gp + tx;
				const uint32_t lo = src[0], hi = (tx + 1u < gp) ? src[1] : 0u;
				val = __builtin_amdgcn_alignbit(hi, lo, g.m_xoff);       // bit x of the row = pixel x
			}
			wv[q] = val; any |= val;
		}
		const unsigned long long bal = __ballot(active && any != 0u);
		const uint32_t in_a = (uint32_t)__popcll(two ? (bal & 0xFFFFFFFFull) : bal);   // non-empty tiles of the first (or only) row of the step
		const unsigned long long mine = two ? (sub ? bal >> 32 : bal & 0xFFFFFFFFull) : bal;
		const uint32_t slot = count + (sub ? in_a : 0u) + (uint32_t)__popcll(mine & ((1ull << k) - 1ull));
		if (active && any != 0u) {
			if (slot < tile_cap) {
#pragma unroll
				for (uint32_t q = 0; q < 8u; ++q) tiles[(slot + 1u) * 8u + q] = wv[q];
			}
			const uint32_t col = tx + 2u;
			atomicOr(rows0 + (ty * G + (col >> 6)) * 4u + ((col & 63u) >> 5), 1u << (col & 31u));
		}
		team_barrier<true>();
		// the entries' bases: tiles before the group's first (lane (row of the step, group) looks after one entry)
		if (lane < step * G) {
			const uint32_t sr = lane / G, gg = lane - sr * G;
			if (r + sr < nty) {
				uint32_t *row = rows0 + (ty0 + r + sr) * G * 4u;
				uint32_t base = count + (sr ? in_a : 0u);
				for (uint32_t h = 0; h < gg; ++h) base += (uint32_t)__builtin_popcount(row[h * 4u]) + (uint32_t)__builtin_popcount(row[h * 4u + 1u]);
				row[gg * 4u + 2u] = base;
			}
		}
		count += (uint32_t)__popcll(bal);
	}
	if (lane == 0) *ntiles = count;
	team_barrier<true>();
	Win &m = v.m;
	v.gbits = gbits;
	m.w = g.rw; m.h = g.rh; m.wf = (float)g.rw; m.hf = (float)g.rh;
	m.p = smem; m.pitch4 = 0u; m.y_lo = 0; m.xbias = 0; m.rows_hi = 0u; m.cols_hi = 0u;
	m.rows0 = nullptr; m.ylo_f = 0.0f; m.yhi_f = 0.0f;
	m.c_p = (const LdsWord *)smem; m.c_y0 = 0u; m.c_rows = 0u; m.c_pitch4 = 0u;
	m.t_idx = nullptr; m.t_tiles = (const LdsWord *)tiles; m.t_pitch = TWP; m.tiled = true;
	m.tc_rows = (const LdsWord *)rows0; m.tc_groups = G; m.compact = true;
	m.w2 = nullptr;
	v.wy0 = aux.y_min; v.wrows = aux.y_max - aux.y_min + 1u; v.wwords = TW; v.xorg = 0;
	v.c_pitch = 0u; v.c_cap_rows = 0u;
	return count <= tile_cap;
}

// ---- ... and behind the compact index (LSD_MODE_TILEC) from the pass's tile-major mask -------------------------------------------
// The compact index numbers the tiles in raster order, so the store is built in three steps: (1) every fetched tile ORs the
// occupancy bits of the (one or two) tiles it feeds into the index; (2) the running counts of the tile rows (a prefix sum over
// the rows, one row per lane); (3) the tiles are fetched again -- 32 bytes each out of the L2 they have just been read into --
// and OR-ed into the slots the finished index gives them (LDS atomics: a tile's two feeders may arrive in the same instruction).
// -> 0 built; 1 more than tile_cap tiles; 2 not usable (more non-empty tiles than `tmp` holds): the caller walks the bit rows
__device__ __forceinline__ uint32_t frame_setup_tilec_occ(const Geom &g, const Buffers &b, uint32_t f, const FrameAux &aux, uint32_t *smem, uint32_t tile_cap, uint32_t *ntiles, FrameView &v,
                                                          uint32_t *tmp, uint32_t tmp_words) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t TW = (g.rw + 31u) >> 5, TWP = tile_idx_pitch(g.rw), gp = g.bits_pitch_w, G = tilec_groups(g.rw), xoff = g.m_xoff;
	uint32_t *tiles = smem;
	uint32_t *idxw = smem + (tile_cap + 1u) * 8u;
	const uint32_t idx_words = tilec_idx_words(g.rw, g.rh);
	for (uint32_t i = lane; i < idx_words; i += 64u) idxw[i] = 0u;
	if (lane < 8u) tiles[lane] = 0u;
	uint32_t *rows0 = idxw + G * 4u;                            // the entry of (tile row 0, group 0)
	// ---- which tiles ----
	const uint32_t ty0 = aux.y_min >> 3, nty = (aux.y_max >> 3) - ty0 + 1u;
	const uint32_t n_g = occ_tile_list(g, b, f, aux, tmp, tmp_words);
	if (n_g > tmp_words) return 2u;
	const uint32_t *tg = b.tiled + (size_t)f * tiled_stride_w(g);
	// one fetched tile -> what it feeds: the tile of its own word column (bits >> xoff) and the one to its left (low xoff bits)
	auto feeds = [&](uint32_t c, const uint4 &lo, const uint4 &hi, uint32_t (&m)[8], uint32_t (&sp)[8], bool &any_m, bool &any_s) {
		const uint32_t ty = c >> 16, wx = c & 0xFFFFu;
		uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
		uint32_t am = 0u, as = 0u;
#pragma unroll
		for (uint32_t r = 0; r < 8u; ++r) {
			if (ty * 8u + r >= g.rh) w[r] = 0u;                     // (the last tile row's rows beyond the image are never written)
			m[r] = w[r] >> xoff; am |= m[r];
			sp[r] = xoff ? w[r] << (32u - xoff) : 0u; as |= sp[r];
		}
		any_m = wx < TW && am != 0u;
		any_s = wx >= 1u && wx - 1u < TW && as != 0u;
	};
	// ---- (1) occupancy ----
	for (uint32_t e0 = 0; e0 < n_g; e0 += 128u) {
#pragma unroll
		for (uint32_t h = 0; h < 2u; ++h) {
			const uint32_t e = e0 + h * 64u + lane;
			if (e < n_g) {
				const uint32_t c = tmp[e];
				const uint4 *src = (const uint4 *)(tg + ((size_t)(c >> 16) * gp + (c & 0xFFFFu)) * 8u);
				const uint4 lo = src[0], hi = src[1];
				uint32_t m[8], sp[8];
				bool any_m, any_s;
				feeds(c, lo, hi, m, sp, any_m, any_s);
				const uint32_t ty = c >> 16, col = (c & 0xFFFFu) + 2u;
				if (any_m) atomicOr(rows0 + (ty * G + (col >> 6)) * 4u + ((col & 63u) >> 5), 1u << (col & 31u));
				if (any_s) atomicOr(rows0 + (ty * G + ((col - 1u) >> 6)) * 4u + (((col - 1u) & 63u) >> 5), 1u << ((col - 1u) & 31u));
			}
		}
	}
	team_barrier<true>();
	// ---- (2) the running counts of tile rows ty0 .. ty0 + nty - 1 ----
	uint32_t count = 0;
	for (uint32_t r0 = 0; r0 < nty; r0 += 64u) {
		const uint32_t r = r0 + lane;
		uint32_t *row = rows0 + (ty0 + min(r, nty - 1u)) * G * 4u;
		uint32_t cnt = 0;
		if (r < nty) for (uint32_t h = 0; h < G; ++h) cnt += (uint32_t)__builtin_popcount(row[h * 4u]) + (uint32_t)__builtin_popcount(row[h * 4u + 1u]);
		uint32_t total;
		uint32_t base = count + wave_excl_prefix32(cnt, lane, &total);
		if (r < nty) for (uint32_t h = 0; h < G; ++h) { row[h * 4u + 2u] = base; base += (uint32_t)__builtin_popcount(row[h * 4u]) + (uint32_t)__builtin_popcount(row[h * 4u + 1u]); }
		count += total;
	}
	if (lane == 0) *ntiles = count;
	Win &m = v.m;
	v.gbits = b.bits + (size_t)f * g.bits_stride_w;
	m.w = g.rw; m.h = g.rh; m.wf = (float)g.rw; m.hf = (float)g.rh;
	m.p = smem; m.pitch4 = 0u; m.y_lo = 0; m.xbias = 0; m.rows_hi = 0u; m.cols_hi = 0u;
	m.rows0 = nullptr; m.ylo_f = 0.0f; m.yhi_f = 0.0f;
	m.c_p = (const LdsWord *)smem; m.c_y0 = 0u; m.c_rows = 0u; m.c_pitch4 = 0u;
	m.t_idx = nullptr; m.t_tiles = (const LdsWord *)tiles; m.t_pitch = TWP; m.tiled = true;
	m.tc_rows = (const LdsWord *)rows0; m.tc_groups = G; m.compact = true;
	m.w2 = nullptr;
	v.wy0 = aux.y_min; v.wrows = aux.y_max - aux.y_min + 1u; v.wwords = TW; v.xorg = 0;
	v.c_pitch = 0u; v.c_cap_rows = 0u;
	if (count > tile_cap) { team_barrier<true>(); return 1u; }
	// ---- (3) the tiles ----
	for (uint32_t i = 8u + lane; i < (count + 1u) * 8u; i += 64u) tiles[i] = 0u;
	team_barrier<true>();
	for (uint32_t e0 = 0; e0 < n_g; e0 += 128u) {
#pragma unroll
		for (uint32_t h = 0; h < 2u; ++h) {
			const uint32_t e = e0 + h * 64u + lane;
			if (e < n_g) {
				const uint32_t c = tmp[e];
				const uint4 *src = (const uint4 *)(tg + ((size_t)(c >> 16) * gp + (c & 0xFFFFu)) * 8u);
				const uint4 lo = src[0], hi = src[1];
				uint32_t mm[8], sp[8];
				bool any_m, any_s;
				feeds(c, lo, hi, mm, sp, any_m, any_s);
				const int ty = (int)(c >> 16), wx = (int)(c & 0xFFFFu);
				if (any_m) {
					uint32_t *t = tiles + tilec_number(m, wx, ty) * 8u;
#pragma unroll
					for (uint32_t r = 0; r < 8u; ++r) if (mm[r]) atomicOr(t + r, mm[r]);
				}
				if (any_s) {
					uint32_t *t = tiles + tilec_number(m, wx - 1, ty) * 8u;
#pragma unroll
					for (uint32_t r = 0; r < 8u; ++r) if (sp[r]) atomicOr(t + r, sp[r]);
				}
			}
		}
	}
	team_barrier<true>();
	return 0u;
}

template <int MODE>
__device__ void lsd_frame_wave(const Geom &g, const Buffers &b, uint32_t f, float max_gap, const FrameAux &aux, uint32_t *smem, WShared &ws, const uint32_t *cull_tab, uint32_t win_cap,
                               uint32_t spin_limit, uint32_t list_cap, const FrameView *tile_view = nullptr, FarmFrame *farm = nullptr) {
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, bs = blockDim.x, nw = bs >> 6;
	smhv_frame_result *res = &b.results[f];
	FrameView v;
	if (MODE == LSD_MODE_TILE) v = *tile_view;           // built by the caller (frame_setup_tile), which also decided that the frame fits
	else frame_setup<MODE>(g, b, f, aux, smem, v);
	const Win &m = v.m;
	uint32_t *list = smem + win_cap, *survw = list + list_cap, *wwins = survw + list_cap;   // wwins: W_NWIN windows
	const uint32_t wy0 = v.wy0, wrows = v.wrows, wwords = v.wwords;
	const int xorg = v.xorg;
	const uint32_t WT = wrows * wwords;
	auto dom_word = [&](uint32_t wi) -> uint32_t {
		const uint32_t r = wi / wwords, c = wi - r * wwords;
		if (MODE == LSD_MODE_TILE) return tile_word(m, (int)c, (int)(wy0 + r));
		return m.p[wi];                                             // LSD_MODE_GLOBAL
	};
	const uint32_t cull = cull_mode_for(b.cull_tab, max_gap);
	const uint32_t epoch = b.co.epoch;
	if (tid == 0) { ws.stuck = 0u; ws.lock = 0u; ws.head = 0u; ws.tail = 0u; ws.spec = 1u; ws.n_lines = 0u; ws.rounds = 0u; ws.frame_done = 0u; ws.steps = 0ull;
	                ws.win_free = (1u << W_NWIN) - 1u; ws.farm_on = 0u; ws.farm_posted = 0u; ws.farm_retired = 0u;
	                ws.late = (farm && (b.lsd_flags & SMH_LSD_LATE_HELP)) ? 1u : 0u; ws.want_set = 0u; ws.want_tick = 0u; ws.t0 = __builtin_amdgcn_s_memtime(); ws.late_cycles = (unsigned long long)b.lsd_late_kc << 10; }
	if (tid < W_ROB) { ws.rob[tid].state = W_FREE; ws.rob[tid].todo = 0ull; }
#ifdef SMH_LSD_WDEBUG
	if (tid < 8) ws.dbg[tid] = 0u;
	if (tid < 4) ws.why[tid] = 0u;
	if (tid < 12) ws.prof[tid] = 0ull;
	if (tid < 8) ws.lat[tid] = 0ull;
#endif
	uint32_t seg_start = 0;
	while (true) {
		// ---- ordered compaction of the non-zero mask words in [seg_start, WT) into `list` (workgroup-wide) ----
		const uint32_t range = WT - seg_start;
		const uint32_t per = (range + bs - 1u) / bs;
		const uint32_t my0 = min(seg_start + tid * per, WT), my1 = min(my0 + per, WT);
		uint32_t cnt = 0;
		for (uint32_t wi = my0; wi < my1; ++wi) cnt += dom_word(wi) != 0u ? 1u : 0u;
		uint32_t incl = cnt;
		for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o); if (lane >= (uint32_t)o) incl += t; }
		if (lane == 63) ws.scan[wave] = incl;
		if (tid == 0) ws.segnext = WT;
		__syncthreads();
		uint32_t wprefix = 0, total = 0;
#pragma unroll
		for (int k = 0; k < LSD_NW; ++k) { const uint32_t s = (uint32_t)k < nw ? ws.scan[k] : 0u; if ((uint32_t)k < wave) wprefix += s; total += s; }
		uint32_t o = wprefix + incl - cnt;
		for (uint32_t wi = my0; wi < my1; ++wi) {
			const uint32_t w = dom_word(wi);
			if (w != 0u) {
				if (o < list_cap) { list[o] = wi; survw[o] = w; ws.stag[o] = 0; }
				else if (o == list_cap) ws.segnext = wi;
				++o;
			}
		}
		if (tid == 0) { ws.disp_e = 0u; ws.disp_end = min(total, list_cap); }
		__syncthreads();
		const uint32_t segnext = ws.segnext;

		// ---- the waves on their own: cast the oldest unclaimed unit; with none to be had, retire / dispatch ----
		uint32_t spins = 0;
#ifdef SMH_LSD_WDEBUG
		unsigned long long wprof[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, wlast = __builtin_amdgcn_s_memtime();
		const unsigned long long wstart = wlast;
#endif
		bool finished_one = false;                                  // this wave has just completed a candidate: retire before anything else
		while (true) {
			uint32_t slot = 0, unit = 0;
			if (!finished_one && claim_unit(ws, slot, unit)) {
				WDBG(0, 1u);
				WPROF(0);
				WSlot &sl = ws.rob[slot];
				#ifdef SMH_LSD_WDEBUG
				const bool last = unit_cast<MODE>(m, wwins + sl.win * W_WIN_STRIDE, b.ray_off, sl, &ws.win_free, unit, max_gap, wprof);
#else
				const bool last = unit_cast<MODE>(m, wwins + sl.win * W_WIN_STRIDE, b.ray_off, sl, &ws.win_free, unit, max_gap);
#endif
				WPROF(1);
				if (last) { finished_one = true; WPROF(2); }
				spins = 0;                                              // progress: the watchdog counts polls WITHOUT any
				continue;
			}
			WPROF(0);
			if (!finished_one) {
				// nothing to cast: is there anything to retire or to dispatch?  (unlocked look; the lock is only worth taking then)
				const uint32_t h0 = W_LD(&ws.head), t0 = W_LD(&ws.tail);
				bool can_retire = false;
				if (h0 != t0) {
					const WSlot &hs = ws.rob[h0 % W_ROB];
					const uint32_t hst = W_LD(&hs.state);
					can_retire = hst == W_DONE || (hst == W_REMOTE && (g_ld64(&farm->ring[hs.win].done) >> 32) == hs.tag);
				}
				const bool can_dispatch = t0 - h0 < W_LD(&ws.spec) && W_LD(&ws.disp_e) < ws.disp_end &&
				                          (W_LD(&ws.win_free) != 0u || (farm && W_LD(&ws.farm_on) && W_LD(&ws.farm_posted) - W_LD(&ws.farm_retired) < SMH_FARM_RING));
				const bool maybe_over = h0 == t0 && W_LD(&ws.disp_e) >= ws.disp_end;
#ifdef SMH_LSD_WDEBUG
				if (lane == 0 && !can_retire && !can_dispatch) {
					atomicAdd(&ws.why[3], 1u);
					if (!(t0 - h0 < W_LD(&ws.spec))) atomicAdd(&ws.why[0], 1u);
					else if (W_LD(&ws.win_free) == 0u) atomicAdd(&ws.why[1], 1u);
					else if (!(W_LD(&ws.disp_e) < ws.disp_end)) atomicAdd(&ws.why[2], 1u);
				}
#endif
				if (!can_retire && !can_dispatch && !maybe_over && !W_LD(&ws.frame_done)) {
					if (++spins > spin_limit) { if (lane == 0) { W_ST(&ws.stuck, 1u); W_ST(&ws.frame_done, 1u); } break; }
					__builtin_amdgcn_s_sleep(16);
					WPROF(6);
					continue;
				}
			}
			finished_one = false;
			// try-lock: somebody else is already retiring / dispatching -- then there will be units to cast in a moment
			uint32_t got_lock = 0;
			if (lane == 0) got_lock = __hip_atomic_exchange(&ws.lock, 1u, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == 0u ? 1u : 0u;
			if (uniform_u32(got_lock) == 0u) {
				if (++spins > spin_limit) { if (lane == 0) { W_ST(&ws.stuck, 1u); W_ST(&ws.frame_done, 1u); } break; }
				__builtin_amdgcn_s_sleep(8);
				WPROF(3);
				continue;
			}
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");     // every lane: nothing of the critical section moves above the lock
			WPROF(3);
			wave_retire<MODE>(m, ws, farm, epoch);
#ifdef SMH_LSD_WDEBUG_SPLIT
			WPROF(4);                                               // (split of "control": bucket 4 = retirement, bucket 2 = dispatch)
#endif
			uint32_t px = 0, py = 0, lines_seen = 0;
			bool got = false;
			const uint32_t head = W_LD(&ws.head), tail = W_LD(&ws.tail);
			const bool fdone = W_LD(&ws.frame_done) != 0u;
			if (!fdone && tail - head < ws.spec) {
				// where the next candidate is cast: here (needs a window) or by the frame's helper workgroup (needs a ring entry);
				// with both to be had, whichever side has fewer candidates in flight
				if (farm && !ws.farm_on && (!ws.late || (ws.want_set && (tail & 3u) == 0u)) && g_ld64(&farm->attached) == (unsigned long long)epoch) {
					if (lane == 0) W_ST(&ws.farm_on, 1u);
					__builtin_amdgcn_wave_barrier();
				}
				const uint32_t wfree = W_LD(&ws.win_free), remote_in = ws.farm_posted - ws.farm_retired;
				const bool can_local = wfree != 0u, can_remote = farm && W_LD(&ws.farm_on) && remote_in < SMH_FARM_RING;
				const uint32_t local_in = W_NWIN - (uint32_t)__popc(wfree);
				const bool remote = can_remote && (!can_local || remote_in < local_in);
				if (can_local || can_remote) got = wave_dispatch(ws, list, survw, wy0, wwords, xorg, px, py);
				if (got) {
					slot = tail % W_ROB;
					lines_seen = W_LD(&ws.n_lines);
					WSlot &sl = ws.rob[slot];
					if (remote) {
						const uint32_t k = ws.farm_posted, ring = k % SMH_FARM_RING;
						if (lane == 0) {
							sl.px = px; sl.py = py; sl.lines_seen = lines_seen; sl.win = ring; sl.tag = farm_done_tag(epoch, k);
#ifdef SMH_LSD_WDEBUG
							sl.t_disp = __builtin_amdgcn_s_memtime();
#endif
							W_ST(&ws.farm_posted, k + 1u);
							g_st64(&farm->ring[ring].post, farm_post_word(epoch, k, px, py));
							W_ST(&sl.state, (uint32_t)W_REMOTE);
							W_ST_REL(&ws.tail, tail + 1u);
						}
						got = false;                                  // nothing to set up here
					} else if (lane == 0) {
						const uint32_t w = (uint32_t)__builtin_ctz(wfree);
						__hip_atomic_fetch_and(&ws.win_free, ~(1u << w), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // (the others only ever ADD bits)
						sl.px = px; sl.py = py; sl.lines_seen = lines_seen; sl.win = w;
#ifdef SMH_LSD_WDEBUG
						sl.t_disp = __builtin_amdgcn_s_memtime(); sl.t_setup = 0ull; sl.t_done = 0ull;
#endif
						W_ST(&sl.state, (uint32_t)W_SETUP);
						W_ST_REL(&ws.tail, tail + 1u);
					}
				}
			}
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
			__builtin_amdgcn_wave_barrier();
			const bool drained = W_LD(&ws.head) == W_LD(&ws.tail) && !got;   // (a candidate posted to the helper has moved the tail)
			const bool exhausted = W_LD(&ws.disp_e) >= ws.disp_end;
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
			if (lane == 0) __hip_atomic_store(&ws.lock, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
#ifdef SMH_LSD_WDEBUG_SPLIT
			WPROF(2);
#else
			WPROF(4);
#endif
			if (got) {
				// the new candidate: start point and live units, then its units are up for grabs (this wave takes part like any other)
				WSlot &sl = ws.rob[slot];
				float xs, ys;
				unsigned long long live;
				cand_setup(m, wwins + uniform_u32(sl.win) * W_WIN_STRIDE, cull_tab, cull, px, py, xs, ys, live);
				WDBG(1, 1u);
#ifdef SMH_LSD_WDEBUG
				if (lane == 0) { sl.t_setup = __builtin_amdgcn_s_memtime(); sl.t_done = sl.t_setup; }
#endif
				if (lane == 0) {
					sl.ptx = xs; sl.pty = ys; sl.live = live; sl.best = 0ull; sl.ex = xs; sl.ey = ys; sl.block = 0u;
					sl.steps = 0u; sl.pending = (uint32_t)__popcll(live);
					if (live) {
						W_ST(&sl.state, (uint32_t)W_CASTING);
						__hip_atomic_store(&sl.todo, live, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
					} else {
						__hip_atomic_fetch_or(&ws.win_free, 1u << sl.win, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
						W_ST_REL(&sl.state, (uint32_t)W_DONE);      // no unit can hold an acceptable ray: rejected as it stands
					}
				}
				finished_one = live == 0ull;
				spins = 0;
				WPROF(5);
				continue;
			}
			if (fdone || (exhausted && drained)) break;
			WDBG(4, 1u);
			if (++spins > spin_limit) {                             // watchdog: never observed; a stuck frame becomes an error record
				if (lane == 0) { W_ST(&ws.stuck, 1u); W_ST(&ws.frame_done, 1u); }
				break;
			}
			__builtin_amdgcn_s_sleep(4);
			WPROF(6);
		}
#ifdef SMH_LSD_WDEBUG
		wprof[7] = __builtin_amdgcn_s_memtime() - wstart;
		if (lane == 0) for (int k = 0; k < 12; ++k) atomicAdd(&ws.prof[k], wprof[k]);
#endif
		__syncthreads();
#ifdef SMH_LSD_WDEBUG
		if (tid < ws.disp_end && survw[tid] != 0u) atomicAdd(&ws.dbg[1], 1u);
		__syncthreads();
#endif
		if (ws.frame_done || segnext >= WT) break;
		seg_start = segnext;
		__syncthreads();
	}
	if (farm && tid == 0) g_st64(&farm->owner_done, (unsigned long long)epoch);   // the helper leaves
	const uint32_t n_lines = ws.n_lines;
	if (tid < n_lines) {
		res->lines[tid].x0 = ws.lines[tid][0]; res->lines[tid].y0 = ws.lines[tid][1];
		res->lines[tid].x1 = ws.lines[tid][2]; res->lines[tid].y1 = ws.lines[tid][3];
	}
	if (tid == 0) { res->n_lines = n_lines; res->rounds = ws.rounds; res->ray_steps = ws.steps; res->status = SMHV_FRAME_OK; }
	if (ws.stuck && tid == 0) {
		// error record (smh_vision_hip.h, SMHV_FRAME_LSD_STUCK): no lines, rounds = 0xFFFFFFFF, status set; the first such
		// frame of the batch leaves the scheduler's state in the batch's error mailbox (host memory) for the message
		res->n_lines = 0; res->rounds = 0xFFFFFFFFu; res->status = SMHV_FRAME_LSD_STUCK;
		BatchError *er = b.err;
		if (er && __hip_atomic_fetch_add(&er->count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0u) {
			er->frame = f; er->status = SMHV_FRAME_LSD_STUCK;
			er->info[0] = ws.head; er->info[1] = ws.tail; er->info[2] = ws.disp_e; er->info[3] = ws.disp_end;
			er->info[4] = ws.n_lines; er->info[5] = ws.rounds; er->info[6] = ws.spec; er->info[7] = ws.rob[ws.head % W_ROB].state;
			__threadfence_system();
		}
	}
#ifdef SMH_LSD_WDEBUG
	if (tid < 4) res->meters[28 + tid] = (double)ws.dbg[tid];
	if (tid < 8) res->meters[20 + tid] = (double)ws.prof[tid];
	if (tid < 4) res->angle[16 + tid] = (float)ws.prof[8 + tid];
	if (tid < 4) res->length_px[28 + tid] = (double)ws.lat[tid];
	if (tid < 4) res->length_px[22 + tid] = (double)ws.lat[4 + tid];
	if (tid < 4) res->angle[20 + tid] = (float)ws.why[tid];
	if (tid == 0) { res->length_px[27] = (double)ws.farm_retired; res->length_px[26] = (double)ws.farm_on; }
#endif
}


// A helper workgroup (blockIdx >= the launch's frame count): the same waves-claim-units machinery on the tile store of the
// frame it attached to, fed by the candidates the frame's owner posts (FarmEntry::post) instead of a raster scan, and
// "retiring" a candidate means sending its result back.  It never accepts a line, counts a round or touches a record.
template <int MODE>
__device__ void lsd_frame_help(const Buffers &b, float max_gap, uint32_t *smem, WShared &ws, const uint32_t *cull_tab, uint32_t win_cap, uint32_t spin_limit, uint32_t list_cap,
                               const FrameView &v, FarmFrame *farm) {
	const uint32_t tid = threadIdx.x, lane = tid & 63u;
	const Win &m = v.m;
	uint32_t *wwins = smem + win_cap + 2u * list_cap;
	const uint32_t cull = cull_mode_for(b.cull_tab, max_gap);
	const uint32_t epoch = b.co.epoch;
	if (tid == 0) { ws.lock = 0u; ws.head = 0u; ws.tail = 0u; ws.win_free = (1u << W_NWIN) - 1u; ws.farm_posted = 0u; ws.frame_done = 0u; }
	if (tid < W_ROB) { ws.rob[tid].state = W_FREE; ws.rob[tid].todo = 0ull; }
	__syncthreads();
	if (tid == 0) g_st64(&farm->attached, (unsigned long long)epoch);          // listening
	uint32_t spins = 0;
	bool finished_one = false;
	while (true) {
		uint32_t slot = 0, unit = 0;
		if (!finished_one && claim_unit(ws, slot, unit)) {
			WSlot &sl = ws.rob[slot];
#ifdef SMH_LSD_WDEBUG
			unsigned long long wprof[12];
			const bool last = unit_cast<MODE>(m, wwins + sl.win * W_WIN_STRIDE, b.ray_off, sl, &ws.win_free, unit, max_gap, wprof);
#else
			const bool last = unit_cast<MODE>(m, wwins + sl.win * W_WIN_STRIDE, b.ray_off, sl, &ws.win_free, unit, max_gap);
#endif
			if (last) finished_one = true;
			spins = 0;
			continue;
		}
		const uint32_t k_next = W_LD(&ws.farm_posted);                          // posts taken so far
		if (!finished_one) {
			const uint32_t h0 = W_LD(&ws.head), t0 = W_LD(&ws.tail);
			const bool can_retire = h0 != t0 && W_LD(&ws.rob[h0 % W_ROB].state) == W_DONE;
			const unsigned long long pw = g_ld64(&farm->ring[k_next % SMH_FARM_RING].post);
			const bool can_fetch = W_LD(&ws.win_free) != 0u && (pw >> 24) == (farm_post_word(epoch, k_next, 0u, 0u) >> 24);
			if (!can_retire && !can_fetch) {
				if (h0 == t0 && g_ld64(&farm->owner_done) == (unsigned long long)epoch) break;   // the owner has finished: nothing more will come
				if (++spins > spin_limit) break;                                              // (an owner that never finishes: leave)
				__builtin_amdgcn_s_sleep(16);
				continue;
			}
		}
		finished_one = false;
		uint32_t got_lock = 0;
		if (lane == 0) got_lock = __hip_atomic_exchange(&ws.lock, 1u, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == 0u ? 1u : 0u;
		if (uniform_u32(got_lock) == 0u) { __builtin_amdgcn_s_sleep(8); continue; }
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
		// ---- send back what is finished, in order ----
		uint32_t head = W_LD(&ws.head);
		const uint32_t tail = W_LD(&ws.tail);
		while (head != tail) {
			WSlot &sl = ws.rob[head % W_ROB];
			if (W_LD_ACQ(&sl.state) != W_DONE) break;
			if (lane == 0) {
				FarmEntry *e = &farm->ring[(uint32_t)(sl.tag >> 32)];
				g_st64(&e->best, sl.best);
				g_st64(&e->end, ((unsigned long long)__float_as_uint(sl.ey) << 32) | __float_as_uint(sl.ex));
				g_st64(&e->start, ((unsigned long long)__float_as_uint(sl.pty) << 32) | __float_as_uint(sl.ptx));
				asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // the payload has left before the tag does
				g_st64(&e->done, ((unsigned long long)(uint32_t)sl.tag << 32) | sl.steps);
				W_ST(&sl.state, (uint32_t)W_FREE);
			}
			++head;
		}
		if (lane == 0) W_ST(&ws.head, head);
		// ---- take the next posted candidate ----
		bool got = false;
		uint32_t px = 0, py = 0;
		const uint32_t k = W_LD(&ws.farm_posted), wfree = W_LD(&ws.win_free);
		if (wfree != 0u) {
			const unsigned long long pw = g_ld64(&farm->ring[k % SMH_FARM_RING].post);
			if ((pw >> 24) == (farm_post_word(epoch, k, 0u, 0u) >> 24)) {
				got = true;
				px = (uint32_t)pw & 0xFFFu; py = (uint32_t)(pw >> 12) & 0xFFFu;
				slot = tail % W_ROB;
				if (lane == 0) {
					WSlot &sl = ws.rob[slot];
					const uint32_t w = (uint32_t)__builtin_ctz(wfree);
					__hip_atomic_fetch_and(&ws.win_free, ~(1u << w), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // (the others only ever ADD bits)
					sl.px = px; sl.py = py; sl.win = w;
					sl.tag = ((unsigned long long)(k % SMH_FARM_RING) << 32) | farm_done_tag(epoch, k);   // (ring entry, tag)
					W_ST(&ws.farm_posted, k + 1u);
					W_ST(&sl.state, (uint32_t)W_SETUP);
					W_ST_REL(&ws.tail, tail + 1u);
				}
			}
		}
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
		if (lane == 0) __hip_atomic_store(&ws.lock, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
		if (got) {
			WSlot &sl = ws.rob[slot];
			float xs, ys;
			unsigned long long live;
			cand_setup(m, wwins + uniform_u32(sl.win) * W_WIN_STRIDE, cull_tab, cull, px, py, xs, ys, live);
			if (lane == 0) {
				sl.ptx = xs; sl.pty = ys; sl.live = live; sl.best = 0ull; sl.ex = xs; sl.ey = ys; sl.block = 0u;
				sl.steps = 0u; sl.pending = (uint32_t)__popcll(live);
				if (live) {
					W_ST(&sl.state, (uint32_t)W_CASTING);
					__hip_atomic_store(&sl.todo, live, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
				} else {
					__hip_atomic_fetch_or(&ws.win_free, 1u << sl.win, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
					W_ST_REL(&sl.state, (uint32_t)W_DONE);
				}
			}
			finished_one = live == 0ull;
			spins = 0;
		}
	}
}

// Late helpers: a workgroup that has finished its own frame looks ONCE for a frame that has asked for help (FarmFrame::want,
// this launch's epoch, nobody's yet), takes the one with the most list entries left (compare-and-swap on `claimed`), builds
// that frame's tile store and serves its owner like a static helper until the owner is done.  Workgroup-wide; -> frame or ~0.
__device__ __forceinline__ uint32_t late_pick(const Buffers &b, uint32_t n_frames, uint32_t self, WShared &ws) {
	const uint32_t epoch = b.co.epoch;
	const unsigned long long tag = (unsigned long long)(epoch & 0xFFFFu) << 48;
	for (uint32_t attempt = 0; attempt < 3u; ++attempt) {
		if (threadIdx.x == 0) ws.pick = 0u;
		__syncthreads();
		uint32_t key = 0u;                                      // (left + 1) << 12 | frame, 0 = none
		for (uint32_t f = threadIdx.x; f < n_frames; f += blockDim.x) {
			if (f == self) continue;
			const unsigned long long w = g_ld64(&b.farm[f].want);
			if ((w & 0xFFFF000000000000ull) != tag) continue;
			const uint32_t left = (uint32_t)min(w & 0xFFFFFFFFull, 0xFFFFEull);
			if (left < LATE_MIN_LEFT) continue;
			if (g_ld64(&b.farm[f].claimed) == (unsigned long long)epoch || g_ld64(&b.farm[f].owner_done) == (unsigned long long)epoch) continue;
			key = max(key, ((left + 1u) << 12) | (f & 0xFFFu));
		}
		key = wave_max32_dpp(key);
		if ((threadIdx.x & 63u) == 0u && key) atomicMax(&ws.pick, key);
		__syncthreads();
		const uint32_t best = ws.pick;
		__syncthreads();
		if (!best) return 0xFFFFFFFFu;
		const uint32_t f = best & 0xFFFu;
		if (threadIdx.x == 0) {
			unsigned long long expect = g_ld64(&b.farm[f].claimed);
			bool won = false;
			if (expect != (unsigned long long)epoch)
				won = __hip_atomic_compare_exchange_strong(&b.farm[f].claimed, &expect, (unsigned long long)epoch, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			ws.pick = won ? 1u : 0u;
		}
		__syncthreads();
		const bool won = ws.pick != 0u;
		__syncthreads();
		if (won) return f;
	}
	return 0xFFFFFFFFu;
}

// (A real call: inlined beside the tile path, the two instantiations of the search spill each other's registers.  The callee
// reads the launch parameters from the kernel argument segment itself, so the kernel need not keep copies of them in scratch.)
struct TileKernelArgs { Geom g; Buffers b; float max_gap; uint32_t tile_cap; uint32_t spin_limit; uint32_t list_cap; uint32_t n_frames; };
__device__ __attribute__((noinline)) void lsd_frame_global(const TileKernelArgs *ka, uint32_t f, uint32_t *smem, WShared *wsp, const uint32_t *cull_tab) {
	const Geom g = ka->g;
	const Buffers b = ka->b;
	const FrameAux aux = b.aux[f];
	lsd_frame_wave<LSD_MODE_GLOBAL>(g, b, f, ka->max_gap, aux, smem, *wsp, cull_tab, 0u, ka->spin_limit, ka->list_cap);
}

// find_lines on the tile store: every searched frame of the launch, whatever its bounding box.  A frame with more than
// tile_cap non-empty tiles (never seen outside the tests, which lower the cap) is searched right here on the mask in global
// memory, with no LDS copy at all: slow, but a second launch for such frames would sit on every batch's critical path
// (0.23 ms of scheduling latency per pass when four batches are in flight, for workgroups that only look at a flag and leave).
#define LSD_TILE_BS 1024
__global__ void __launch_bounds__(LSD_TILE_BS) __attribute__((amdgpu_waves_per_eu(W_WAVES_PER_EU, W_WAVES_PER_EU))) k_lsd_tile(Geom g, Buffers b, float max_gap, uint32_t tile_cap, uint32_t spin_limit, uint32_t list_cap, uint32_t n_frames) {
	extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
	__shared__ WShared ws;
	__shared__ uint32_t cull_tab[SMH_CULL_TAB_WORDS];
#ifdef SMH_LSD_FAT
	asm volatile("; register footprint experiment" ::: SMH_LSD_FAT);   // e.g. -DSMH_LSD_FAT='"v135"': 136 VGPRs allocated, at most 3 waves per SIMD
#endif
	const uint32_t cull = cull_mode_for(b.cull_tab, max_gap);
	const uint32_t f = blockIdx.x;
	const FrameAux aux = b.aux[f];
	const TileKernelArgs *ka = (const TileKernelArgs *)__builtin_amdgcn_kernarg_segment_ptr();   // (the kernel's own parameter list)
	const bool record = (b.rec_stages & SMH_REC_ON) != 0u;       // this workgroup also writes its frame's record (smh_record.inc)
	if (!aux.open || aux.n_mask_px == 0) {
		if (threadIdx.x == 0) { b.results[f].n_lines = 0; b.results[f].rounds = 0; b.results[f].ray_steps = 0; b.results[f].status = SMHV_FRAME_OK; }
		if (record) { __syncthreads(); frame_record_tail(&ka->g, &ka->b, f); }
		return;
	}
	if (cull) for (uint32_t i = threadIdx.x; i < SMH_CULL_TAB_WORDS; i += blockDim.x) cull_tab[i] = b.cull_tab[i];   // visible after the barriers of the tile build
	// late helpers: the frame's exchange with a workgroup that has finished its own frame
	const bool late = b.farm && (b.lsd_flags & SMH_LSD_LATE_HELP) && n_frames <= 4096u;
	FarmFrame *farm = late ? &b.farm[f] : nullptr;
	FrameView v;
	if (frame_setup_tile(g, b, f, aux, smem, tile_cap, &ws.ntiles, v)) lsd_frame_wave<LSD_MODE_TILE>(g, b, f, max_gap, aux, smem, ws, cull_tab, tile_mask_words(g.rw, g.rh, tile_cap), spin_limit, list_cap, &v, farm);
	else lsd_frame_global(ka, f, smem, &ws, cull_tab);
	if (record) { __syncthreads(); frame_record_tail(&ka->g, &ka->b, f); }   // lines, rounds, status are written: scale ratio + derived outputs
	if (late) {
		__syncthreads();
		const uint32_t t = late_pick(b, n_frames, f, ws);
		if (t == 0xFFFFFFFFu) return;
		const FrameAux aux_t = b.aux[t];
		FrameView vt;
		if (!frame_setup_tile(g, b, t, aux_t, smem, tile_cap, &ws.ntiles, vt)) return;   // (its owner searches in global memory and never asked)
		if (g_ld64(&b.farm[t].owner_done) == (unsigned long long)b.co.epoch) return;      // finished meanwhile
		lsd_frame_help<LSD_MODE_TILE>(b, max_gap, smem, ws, cull_tab, tile_mask_words(g.rw, g.rh, tile_cap), spin_limit, list_cap, vt, &b.farm[t]);
	}
}
