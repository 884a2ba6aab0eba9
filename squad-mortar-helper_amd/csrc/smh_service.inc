// smh_service.inc -- k_lsd_service: the FRAME-GRANULAR line search of a pipeline (included by smh_lsd.hip after
// smh_lsd_seq.inc, whose one-wave-per-frame scan it runs; structures in smh_kernels.h, "the frame-granular line search").
//
// The reference hands a frame's lines back the moment that frame is done (src/vision/mod.rs:219-240).  A batch-granular search
// launch cannot: it lasts as long as its slowest frame (157 rounds against a mean of 53 on the synthetic scene, 372 against 76
// on the reference's screenshots), the batch's slot is blocked until then, and the cheapest search -- one wave per frame, a
// third of the task kernel's wave-time (smh_lsd_seq.inc) -- was unusable because its slowest frame takes four times as long.
// Here the search is decoupled from the batch launch: ONE long-lived kernel per pipeline, whose waves pull (slot, frame) items
// from a ring, each wave on its own -- a workgroup is only the unit that shares the 14.4 KB sector table -- and every frame
// writes its own record and counts itself off against its submission.  Nothing waits for a slowest frame except the slot
// that holds it.
//
// Memory model.  The kernel outlives the kernels whose outputs it reads (the streaming passes of later submissions), so the
// kernel-boundary acquire / release HIP normally provides is done by hand: after claiming an item a wave invalidates its
// vector L1 / the XCD's L2 (agent-scope acquire) AND the scalar data cache (descriptor and aux loads are scalar loads); before
// counting a frame off it writes its L2 back (agent-scope release), so that the records are in memory when the host -- or the
// next kernel -- is told.
#pragma once

struct SvcKernelArgs { Geom g; SvcParams p; };
#ifdef __HIP_DEVICE_COMPILE__
typedef const __attribute__((address_space(4))) SvcSlot *SvcSlotPtr;     // constant address space: scalar loads (the wave invalidates the scalar cache per item)
typedef const __attribute__((address_space(4))) SvcKernelArgs *SvcKernelArgsPtr;
#else
typedef const SvcSlot *SvcSlotPtr;
typedef const SvcKernelArgs *SvcKernelArgsPtr;
#endif
// the kernel argument segment's address as a callee sees it: handed down in vector registers, moved back to a scalar pair
__device__ __forceinline__ SvcKernelArgsPtr svc_args(const void *ka) {
	const unsigned long long v = (unsigned long long)(uintptr_t)ka;
	const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
	return (SvcKernelArgsPtr)(uintptr_t)(((unsigned long long)hi << 32) | lo);
}

#define SVC_WS_WORDS ((uint32_t)((sizeof(WShared) + 15u) / 16u * 4u))
#define SVC_POLL_SLEEP 64               // s_sleep argument of an idle poll (64 x 64 cycles: 1.7 us)

__device__ __forceinline__ uint32_t svc_ld(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// (Real calls: the tile path and the global-memory path would otherwise spill each other's registers.  What the callee needs
// arrives as wave-uniform 32-bit values -- slot, frame, the LDS byte offsets of the wave's block and of the sector table -- and is
// moved to scalar registers first thing; the launch parameters come from the kernel argument segment and the slot's descriptor
// through the constant address space: scalar loads, nothing uniform in vector registers.)
__device__ __forceinline__ uint32_t *lds_ptr(uint32_t byte_off) { return (uint32_t *)(LdsWord *)(uintptr_t)uniform_u32(byte_off); }
__device__ __forceinline__ uint32_t lds_off(const void *p) { return (uint32_t)(uintptr_t)(const LdsByte *)p; }

// (COMPACT only says which of the two service kernels calls this copy: each kernel has callees of its own, compiled to its register budget)
template <bool COMPACT>
__device__ __attribute__((noinline)) void svc_frame_global(const void *kargs, uint32_t slot, uint32_t f, uint32_t part_off, uint32_t cull_off, uint32_t dirs_off) {
	SvcKernelArgsPtr ka = svc_args(kargs);
	slot = uniform_u32(slot); f = uniform_u32(f);
	uint32_t *part = lds_ptr(part_off);
	const Geom g = ka->g;
	const Buffers b = ((SvcSlotPtr)(ka->p.slots + slot))->b;
	const FrameAux aux = b.aux[f];
	lsd_frame_seq<LSD_MODE_GLOBAL, true, false, SVC_WIN_REUSE(COMPACT), SVC_LEAN_SAMPLER(COMPACT)>(g, b, f, ka->p.max_gap, aux, part + SVC_WS_WORDS, *(WShared *)part, lds_ptr(cull_off), (const RayDir *)lds_ptr(dirs_off), 0u, ka->p.list_cap);
}

// -> s_memtime at the end of the search proper (before the record)
// COMPACT: the frame's tile store behind the compact index (LSD_MODE_TILEC; SvcParams::compact: frame sizes where the 16-bit
// table would cost a wave of the workgroup its place)
template <bool COMPACT>
__device__ __attribute__((noinline)) unsigned long long svc_frame(const void *kargs, uint32_t slot, uint32_t f, uint32_t part_off, uint32_t cull_off, uint32_t dirs_off) {
	SvcKernelArgsPtr ka = svc_args(kargs);
	slot = uniform_u32(slot); f = uniform_u32(f);
	uint32_t *part = lds_ptr(part_off);
	const Geom g = ka->g;
	const Buffers b = ((SvcSlotPtr)(ka->p.slots + slot))->b;
	const FrameAux aux = b.aux[f];
	WShared &ws = *(WShared *)part;
	uint32_t *smem = part + SVC_WS_WORDS;
	if (!aux.open || aux.n_mask_px == 0) {
		if ((threadIdx.x & 63u) == 0) { b.results[f].n_lines = 0; b.results[f].rounds = 0; b.results[f].ray_steps = 0; b.results[f].status = SMHV_FRAME_OK; }
	} else {
		const uint32_t tile_cap = ka->p.tile_cap;
		if ((threadIdx.x & 63u) == 0) {                              // (what the frame's request to other workgroups goes by: smh_lsd_seq.inc)
			SvcSlot *sl = ka->p.slots + slot;
			ws.rem_done = (unsigned long long)(uintptr_t)&sl->done;
			ws.rem_n = __hip_atomic_load(&sl->n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
		FrameView v;
		bool fits;
		if constexpr (COMPACT) {
			uint32_t rc = 2u;
			if (b.tiled && aux.tiles && !(ka->p.flags & 32u)) rc = frame_setup_tilec_occ(g, b, f, aux, smem, tile_cap, &ws.ntiles, v, smem + tilec_mask_words(g.rw, g.rh, tile_cap), 2u * ka->p.list_cap + SVC_WIN_STRIDE(true));
			fits = rc == 2u ? frame_setup_tilec(g, b, f, aux, smem, tile_cap, &ws.ntiles, v) : rc == 0u;
		} else {
			// from the tile-major mask the pass left (2-3 round trips); the walk over the bit rows' bounding box when there is none
			uint32_t rc = 2u;
			if (b.tiled && aux.tiles && !(ka->p.flags & 32u)) rc = frame_setup_tile_occ(g, b, f, aux, smem, tile_cap, &ws.ntiles, v, smem + tile_mask_words(g.rw, g.rh, tile_cap), 2u * ka->p.list_cap + SVC_WIN_STRIDE(false));
			fits = rc == 2u ? frame_setup_tile<true>(g, b, f, aux, smem, tile_cap, &ws.ntiles, v) : rc == 0u;
		}
		if (fits) {
			if constexpr (COMPACT) lsd_frame_seq<LSD_MODE_TILEC, true, true, SVC_WIN_REUSE(true)>(g, b, f, ka->p.max_gap, aux, smem, ws, lds_ptr(cull_off), (const RayDir *)lds_ptr(dirs_off), tilec_mask_words(g.rw, g.rh, tile_cap), ka->p.list_cap, &v);
			else lsd_frame_seq<LSD_MODE_TILE, true, true, SVC_WIN_REUSE(false), SVC_LEAN_SAMPLER(false)>(g, b, f, ka->p.max_gap, aux, smem, ws, lds_ptr(cull_off), (const RayDir *)lds_ptr(dirs_off), tile_mask_words(g.rw, g.rh, tile_cap), ka->p.list_cap, &v);
		} else svc_frame_global<COMPACT>(kargs, slot, f, part_off, cull_off, dirs_off);
	}
	const unsigned long long t_search_end = __builtin_amdgcn_s_memtime();
	if (b.rec_stages & SMH_REC_ON) frame_record_tail_wave(&((const SvcKernelArgs *)kargs)->g, &((const SvcSlot *)(ka->p.slots + slot))->b, f);
	return t_search_end;
}

// A wave between two frames of its own serves a wave of its workgroup whose frame has asked for help (smh_lsd_seq.inc, "the
// help desk"): it casts the candidates the owner has posted, on the owner's mask tiles and in its own window block, until
// the owner's frame is done or nothing has been posted for a while.
#define SVC_HELP_IDLE_POLLS 160u        // x ~0.25 us without a post: back to frames of its own
template <bool COMPACT>
__device__ __attribute__((noinline)) void svc_help(const void *kargs, uint32_t owner_off, uint32_t my_off, uint32_t cull_off, uint32_t dirs_off) {
	SvcKernelArgsPtr ka = svc_args(kargs);
	uint32_t *opart = lds_ptr(owner_off), *mpart = lds_ptr(my_off);
	WShared &wo = *(WShared *)opart;
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t ok = 0;
	if (lane == 0 && W_LD_ACQ(&wo.want_set) && W_LD(&wo.late) < SEQ_MAX_HELPERS) {
		const uint32_t prev = __hip_atomic_fetch_add(&wo.late, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
		if (prev < SEQ_MAX_HELPERS && W_LD_ACQ(&wo.want_set)) ok = 1u;
		else __hip_atomic_fetch_sub(&wo.late, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);   // (the owner has finished meanwhile, or the desk is full)
	}
	if (!uniform_u32(ok)) return;
	const uint32_t rw = ka->g.rw, rh = ka->g.rh, tile_cap = ka->p.tile_cap, list_cap = ka->p.list_cap;
	const float max_gap = ka->p.max_gap;
	const uint32_t cull = cull_mode_for(ka->p.cull_tab, max_gap);
	const float *ray_off = ka->p.ray_off;
	Win m;
	if constexpr (COMPACT) tilec_win(m, rw, rh, opart + SVC_WS_WORDS, tile_cap); else tile_win(m, rw, rh, opart + SVC_WS_WORDS, tile_cap);
	uint32_t *wwin = mpart + SVC_WS_WORDS + (COMPACT ? tilec_mask_words(rw, rh, tile_cap) : tile_mask_words(rw, rh, tile_cap)) + 2u * list_cap;
	const uint32_t *cull_tab = lds_ptr(cull_off);
	const RayDir *dirs = (const RayDir *)lds_ptr(dirs_off);
	uint32_t idle = 0;
	// The window this wave keeps between the casts of ONE attach: invalid at entry (whatever the block holds is of another frame),
	// and every cast below is for the same frame of the owner.  Proof: this wave is counted in wo.late from the attach above to
	// the fetch_sub at the end of this function, and the owner ends its frame with `want_set = 0; wait until late == 0`
	// (lsd_frame_seq) BEFORE it writes its next frame's tile store.  The attach raised `late` and then saw want_set != 0, so the
	// owner had not passed that wait -- had it passed, it would have found late != 0 -- and it cannot pass it while this wave
	// is counted.  The same argument is what lets a helper read the owner's tiles at all; the window does not rest on it alone:
	// the tag is keyed by the owner's frame counter (WShared::frame_no, raised at the start of every frame), read with every post
	// taken -- one LDS read per cast -- and a window of another frame is never reused.
	WinTag wtag = {0, 0, false};
	uint32_t wframe = 0u;
	while (uniform_u32(W_LD_ACQ(&wo.want_set))) {
		// the oldest post nobody has taken
		uint32_t key = 0u;                                      // ~(running number << 2 | entry), 0 = none
		if (lane < SEQ_HELP_SLOTS && W_LD_ACQ(&wo.rob[lane].state) == (uint32_t)H_POSTED) key = ~((wo.rob[lane].lines_seen << 2) | lane);
		key = wave_max32_dpp(key);
		if (!key) {
			if (++idle > SVC_HELP_IDLE_POLLS) break;
			__builtin_amdgcn_s_sleep(8);
			continue;
		}
		WSlot &sl = wo.rob[~key & 3u];
		uint32_t got = 0;
		if (lane == 0) { uint32_t expect = H_POSTED; got = __hip_atomic_compare_exchange_strong(&sl.state, &expect, (uint32_t)H_TAKEN, __ATOMIC_ACQ_REL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) ? 1u : 0u; }
		if (!uniform_u32(got)) continue;                        // (the owner took it back, or another helper was quicker)
		idle = 0;
		const uint32_t px = uniform_u32(sl.px), py = uniform_u32(sl.py);
		if (SVC_WIN_REUSE(COMPACT)) {
			const uint32_t oframe = uniform_u32(W_LD(&wo.frame_no));
			if (oframe != wframe) { wframe = oframe; wtag.valid = false; }
		}
		float xs, ys, ex0, ey0;
		unsigned long long wkey;
		uint32_t st_sum;
#ifdef SMH_LSD_WDEBUG
		unsigned long long sprof[8] = {0, 0, 0, 0, 0, 0, 0, 0}, slast = __builtin_amdgcn_s_memtime(), uprof[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
		uint32_t n_units = 0;
		seq_cast_candidate<COMPACT ? LSD_MODE_TILEC : LSD_MODE_TILE, SVC_WIN_REUSE(COMPACT), SVC_LEAN_SAMPLER(COMPACT)>(m, wwin, &wtag, cull_tab, cull, dirs, ray_off, max_gap, px, py, xs, ys, wkey, ex0, ey0, st_sum, sprof, slast, uprof, n_units);
#else
		seq_cast_candidate<COMPACT ? LSD_MODE_TILEC : LSD_MODE_TILE, SVC_WIN_REUSE(COMPACT), SVC_LEAN_SAMPLER(COMPACT)>(m, wwin, &wtag, cull_tab, cull, dirs, ray_off, max_gap, px, py, xs, ys, wkey, ex0, ey0, st_sum);
#endif
		if (lane == 0) {
			sl.ptx = xs; sl.pty = ys; sl.best = wkey; sl.ex = ex0; sl.ey = ey0; sl.steps = st_sum;
			W_ST_REL(&sl.state, (uint32_t)H_DONE);
		}
	}
	if (lane == 0) __hip_atomic_fetch_sub(&wo.late, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// A wave between two frames of its own that has popped a help ticket (smh_kernels.h, "help across workgroups"): it attaches to
// the request the ticket names, copies the owner's tile store into its own LDS block and casts the candidates the owner posts
// in its ring until the request closes or nothing it could take has been posted for a while.
#define SVC_REMOTE_IDLE_POLLS 12u       // x ~2 us: polls without a post to take before a helper leaves while frames are waiting for a wave ...
#define SVC_REMOTE_IDLE_POLLS_FREE 600u // ... and while none is
#define SVC_REMOTE_MAX_HELPERS 12u
template <bool COMPACT>
__device__ __attribute__((noinline)) void svc_help_remote(const void *kargs, uint32_t ticket, uint32_t my_off, uint32_t cull_off, uint32_t dirs_off) {
	SvcKernelArgsPtr ka = svc_args(kargs);
	ticket = uniform_u32(ticket);
	const uint32_t owner = ticket & 0xFFFFu, gen16 = ticket >> 16;
	SvcRemote *r = ka->p.remote + owner;
	const uint32_t lane = threadIdx.x & 63u;
	// ---- attach: only to the request the ticket was issued for, and only while it is open ----
	uint32_t ok = 0, gen = 0;
	if (lane == 0) {
		unsigned long long st = g_ld64(&r->state);
		while ((st & SVC_REMOTE_OPEN) && ((uint32_t)(st >> 32) & 0xFFFFu) == gen16 && ((uint32_t)st & 0x7FFFFFFFu) < SVC_REMOTE_MAX_HELPERS) {
			if (__hip_atomic_compare_exchange_strong(&r->state, &st, st + 1ull, __ATOMIC_ACQ_REL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { ok = 1u; gen = (uint32_t)(st >> 32); break; }
		}
	}
	if (!uniform_u32(ok)) return;
	gen = uniform_u32(gen);
	if (lane == 0) __hip_atomic_fetch_add(&ka->p.ctl->stat_attached, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	// ---- the owner's tile store (written by another CU a moment ago, behind an agent-scope release) ----
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
	const uint32_t rw = ka->g.rw, rh = ka->g.rh, tile_cap = ka->p.tile_cap, list_cap = ka->p.list_cap;
	const uint32_t ntiles = min(uniform_u32((uint32_t)g_ld64(&r->info)), tile_cap);
	uint32_t *mpart = lds_ptr(my_off), *store = mpart + SVC_WS_WORDS;
	{
		const uint4 *src = (const uint4 *)(ka->p.remote_store + (size_t)owner * ka->p.remote_store_words);
		uint4 *dst = (uint4 *)store;
		for (uint32_t i = lane; i < (ntiles + 1u) * 2u; i += 64u) dst[i] = src[i];
		const uint32_t q0 = (tile_cap + 1u) * 2u, nq = ((COMPACT ? tilec_idx_words(rw, rh) : tile_idx_words(rw, rh)) + 3u) / 4u;
		for (uint32_t i = lane; i < nq; i += 64u) dst[q0 + i] = src[q0 + i];
	}
	wave_lds_sync();
	const float max_gap = ka->p.max_gap;
	const uint32_t cull = cull_mode_for(ka->p.cull_tab, max_gap);
	const float *ray_off = ka->p.ray_off;
	Win m;
	if constexpr (COMPACT) tilec_win(m, rw, rh, store, tile_cap); else tile_win(m, rw, rh, store, tile_cap);
	uint32_t *wwin = store + (COMPACT ? tilec_mask_words(rw, rh, tile_cap) : tile_mask_words(rw, rh, tile_cap)) + 2u * list_cap;
	const uint32_t *cull_tab = lds_ptr(cull_off);
	const RayDir *dirs = (const RayDir *)lds_ptr(dirs_off);
	// The window between the casts of this attach: invalid at entry (the store above has just been copied in), and the store is
	// this wave's own copy of ONE request's tiles -- the loop leaves when the request's number changes -- so it stands until the end.
	WinTag wtag = {0, 0, false};
	uint32_t idle = 0, n_cast = 0, n_polls = 0, n_empty = 0, n_lost = 0, exit_idle = 0;
	unsigned long long t_cast = 0ull;
	const unsigned long long t_att = __builtin_amdgcn_s_memtime();
	while (true) {
		++n_polls;
		// one round trip: the request's state, the posts and who has taken what
		const unsigned long long st = g_ld64(&r->state);
		unsigned long long pw = 0ull, cw = 0ull;
		if (lane < SVC_REMOTE_RING) { pw = g_ld64(&r->ring[lane].post); cw = g_ld64(&r->ring[lane].claim); }
		if (!(uniform_u32((uint32_t)st) & (uint32_t)SVC_REMOTE_OPEN) || uniform_u32((uint32_t)(st >> 32)) != gen) break;
		// the oldest post nobody has taken
		const uint32_t pk = (uint32_t)(pw >> 32);
		const bool open_post = lane < SVC_REMOTE_RING && pk != 0u && (unsigned long long)pk > cw;
		const uint32_t key = wave_max32_dpp(open_post ? ~pk : 0u);
		if (!key) {
			// nothing to take: stay while the request is open and no frame is waiting for a wave (the owner posts as its scan
			// moves on); with frames waiting, only for a little while
			const int32_t waiting = (int32_t)uniform_u32((uint32_t)__hip_atomic_load(&ka->p.ctl->avail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
			++n_empty;
			if (++idle > (waiting > 0 ? SVC_REMOTE_IDLE_POLLS : SVC_REMOTE_IDLE_POLLS_FREE)) { exit_idle = 1u; break; }
			if (idle < 4u) __builtin_amdgcn_s_sleep(24); else __builtin_amdgcn_s_sleep(72);
			continue;
		}
		const uint32_t k = ~key;
		const uint32_t e = (uint32_t)__builtin_ctzll(__ballot(open_post && pk == k));
		uint32_t mine = 0;
		if (lane == 0) mine = __hip_atomic_fetch_max(&r->ring[e].claim, (unsigned long long)k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned long long)k ? 1u : 0u;
		if (!uniform_u32(mine)) { ++n_lost; continue; }        // (the owner took it back, or another helper was quicker)
		idle = 0;
		const unsigned long long t_c0 = __builtin_amdgcn_s_memtime();
		const uint32_t pxy = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)pw, (int)e);
		const uint32_t px = pxy & 0xFFFFu, py = pxy >> 16;
		float xs, ys, ex0, ey0;
		unsigned long long wkey;
		uint32_t st_sum;
#ifdef SMH_LSD_WDEBUG
		unsigned long long sprof[8] = {0, 0, 0, 0, 0, 0, 0, 0}, slast = __builtin_amdgcn_s_memtime(), uprof[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
		uint32_t n_units = 0;
		seq_cast_candidate<COMPACT ? LSD_MODE_TILEC : LSD_MODE_TILE, SVC_WIN_REUSE(COMPACT), SVC_LEAN_SAMPLER(COMPACT)>(m, wwin, &wtag, cull_tab, cull, dirs, ray_off, max_gap, px, py, xs, ys, wkey, ex0, ey0, st_sum, sprof, slast, uprof, n_units);
#else
		seq_cast_candidate<COMPACT ? LSD_MODE_TILEC : LSD_MODE_TILE, SVC_WIN_REUSE(COMPACT), SVC_LEAN_SAMPLER(COMPACT)>(m, wwin, &wtag, cull_tab, cull, dirs, ray_off, max_gap, px, py, xs, ys, wkey, ex0, ey0, st_sum);
#endif
		++n_cast;
		t_cast += __builtin_amdgcn_s_memtime() - t_c0;
		if (lane == 0) {
			// the two halves, each one write-through store carrying the post's number: no order between them matters
			SvcRemoteEntry *en = &r->ring[e];
			const rem_u32x4 a = {k, st_sum, (uint32_t)(wkey >> 32), (uint32_t)wkey};
			const rem_u32x4 b = {k, __float_as_uint(ex0), __float_as_uint(ey0), ((uint32_t)(ys * 2.0f) << 16) | ((uint32_t)(xs * 2.0f) & 0xFFFFu)};
			g_st128(en->res_a, a);
			g_st128(en->res_b, b);
		}
	}
	// everything this wave wrote into the ring has left before it counts itself off (the owner's next request resets the ring
	// only when nobody is attached)
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	if (lane == 0) {
		__hip_atomic_fetch_sub(&r->state, 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
		SvcCtl *ctl = ka->p.ctl;
		__hip_atomic_fetch_add(&ctl->stat_remote, n_cast, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		__hip_atomic_fetch_add(&ctl->stat_h_polls, n_polls, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		__hip_atomic_fetch_add(&ctl->stat_h_empty, n_empty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		__hip_atomic_fetch_add(&ctl->stat_h_lost, n_lost, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		__hip_atomic_fetch_add(exit_idle ? &ctl->stat_h_idle_exit : &ctl->stat_h_closed_exit, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		__hip_atomic_fetch_add(&ctl->stat_h_cycles, __builtin_amdgcn_s_memtime() - t_att, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		__hip_atomic_fetch_add(&ctl->stat_h_cast_cycles, t_cast, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

// a wave of this workgroup whose frame has asked for help and has room for another helper -> its LDS block's byte offset, or ~0
__device__ __forceinline__ uint32_t svc_sibling_in_need(uint32_t *smem, uint32_t part_words, uint32_t nw, uint32_t me) {
	for (uint32_t w = 0; w < nw; ++w) {
		if (w == me) continue;
		const WShared &wsib = *(const WShared *)(smem + w * part_words);
		if (uniform_u32(W_LD(&wsib.want_set)) && uniform_u32(W_LD(&wsib.late)) < SEQ_MAX_HELPERS) return lds_off(smem + w * part_words);
	}
	return 0xFFFFFFFFu;
}

// One wave: the next item, or 0xFFFFFFFF when the service has closed.  -> slot << 24 | frame
// (0xFFFFFFFE: nothing to pop, but a wave of the workgroup has asked for help)
// checker: the ONE wave of the launch (workgroup 0, wave 0) that looks after the launch's life cycle when idle.  Every idle
// wave doing that -- a read of host memory over PCIe and a handful of device-scope loads every 50 us, 1024 waves -- cost the
// streaming pass beside them a quarter of its rate.
// (0xFFFFFFFD: a help ticket of another workgroup's frame -> *help_ticket; such frames come before a new frame of the wave's own,
// as the siblings' do: they are the old ones)
__device__ __forceinline__ uint32_t svc_pop(const SvcParams &p, uint32_t *team_smem, uint32_t nw, uint32_t me, bool checker, uint32_t *help_ticket) {
	const uint32_t lane = threadIdx.x & 63u;
	SvcCtl *ctl = p.ctl;
	const unsigned long long t_idle0 = __builtin_amdgcn_s_memtime();
	uint32_t polls = 0;
	while (true) {
		// ONE look at the ring per poll: {items available, epoch of the launch that has closed}
		const unsigned long long look = __hip_atomic_load((const unsigned long long *)&ctl->avail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		// a launch that has closed hands over at once: the items that arrive from now on are the next launch's, which waits
		// behind this one on the search stream (a wave that kept popping while items kept coming would never look at the flag,
		// and run the whole pipeline by itself)
		if ((uint32_t)(look >> 32) == p.epoch) return 0xFFFFFFFFu;
		if (p.remote && ((p.flags & 16u) || (int32_t)(uint32_t)look <= 0)) {
			const unsigned long long hl = __hip_atomic_load((const unsigned long long *)&ctl->help_avail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			if ((int32_t)(uint32_t)hl > 0) {
				uint32_t hgot = 0, ht = 0;
				if (lane == 0) {
					if (__hip_atomic_fetch_sub(&ctl->help_avail, 1, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) > 0) { ht = __hip_atomic_fetch_add(&ctl->help_head, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); hgot = 1u; }
					else __hip_atomic_fetch_add(&ctl->help_avail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				}
				if (uniform_u32(hgot)) {
					ht = uniform_u32(ht);
					const unsigned long long *he = &ctl->help_ring[ht & (SVC_HELP_RING - 1u)];
					unsigned long long hw;
					while ((uint32_t)((hw = __hip_atomic_load(he, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >> 32) != ht / SVC_HELP_RING + 1u) __builtin_amdgcn_s_sleep(2);
					*help_ticket = uniform_u32((uint32_t)hw);
					return 0xFFFFFFFDu;
				}
			}
		}
		uint32_t got = 0, ticket = 0;
		if ((int32_t)(uint32_t)look > 0 && lane == 0) {
			if (__hip_atomic_fetch_sub(&ctl->avail, 1, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) > 0) {
				ticket = __hip_atomic_fetch_add(&ctl->head, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				got = 1u;
			} else __hip_atomic_fetch_add(&ctl->avail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
		got = uniform_u32(got);
		if (got) {
			ticket = uniform_u32(ticket);
			// the entry of this ticket: its publisher may still be writing (publishers of different streams run side by side)
			const unsigned long long *e = p.ring + (ticket & ((1u << p.ring_log2) - 1u));
			const uint32_t gen = (ticket >> p.ring_log2) + 1u;
			unsigned long long w;
			while ((uint32_t)((w = __hip_atomic_load(e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >> 32) != gen) __builtin_amdgcn_s_sleep(2);
			if (lane == 0) __hip_atomic_fetch_add(&ctl->busy, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			return uniform_u32((uint32_t)w);
		}
		// Nothing: sleep before the next look -- 2 us at first, 13 us once the wave has been idle for a while (items come in
		// bursts of a batch every few hundred microseconds; a late start costs the frame nothing against that) -- looking only
		// at the workgroup's own LDS in between (a frame of this workgroup that asks for help)
		// (a wave that has been idle for a few hundred microseconds -- a pipeline whose slots wait for a few heavy frames has
		// hundreds of them -- looks every 54 us: with that many waves at random phases a burst of new frames is still picked up
		// within microseconds, and a thousand idle waves looking every 13 us cost the streaming pass beside them 7 %)
		const uint32_t naps = polls < 8u ? 1u : (polls < 32u ? 4u : 16u);
		for (uint32_t k = 0; k < naps; ++k) {
			if (team_smem && svc_sibling_in_need(team_smem, p.part_words, nw, me) != 0xFFFFFFFFu) return 0xFFFFFFFEu;
			if (polls < 8u) __builtin_amdgcn_s_sleep(SVC_POLL_SLEEP); else __builtin_amdgcn_s_sleep(127);
		}
		++polls;
		// Nothing for a while (the checker wave only): may the service close?  Only the launch the host's state word names may decide that, only when
		// every batch the host has counted is complete, no wave is at work and no item is waiting, and only together with the
		// host: the compare-and-swap fails when a submission has been counted meanwhile, and a submission that finds no launch
		// named launches the next one.  A wave of a launch that is NOT named (it closed a moment ago, or the host has moved on)
		// just leaves.  idle_long without any wave at work and with batches outstanding: the streaming side is not moving (its
		// queue blocked behind this kernel?): give way; the host's waits launch the service again.
		if (checker && polls >= 8u && (polls & 3u) == 0u) {
			const unsigned long long idle = (__builtin_amdgcn_s_memtime() - t_idle0) >> 10;
			if (idle >= p.idle_short) {
				uint32_t leave = 0;
				if (lane == 0) {
					unsigned long long st = __hip_atomic_load(&p.host->state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
					if ((uint32_t)st != p.epoch) {                      // not (or no longer) the launch the host counts on: everybody out
						__hip_atomic_store(&ctl->closing, p.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
						leave = 1u;
					} else {
						const uint32_t comp = __hip_atomic_load(&ctl->completed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
						const bool quiet = svc_ld(&ctl->busy) == 0u && __hip_atomic_load(&ctl->avail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= 0;
						const bool drained = quiet && (int32_t)(comp - (uint32_t)(st >> 32)) >= 0;   // (>=: a submission the host un-counted after its items had gone in)
						const bool stalled = quiet && idle >= p.idle_long;
						if ((drained || stalled) &&
						    __hip_atomic_compare_exchange_strong(&p.host->state, &st, st & 0xFFFFFFFF00000000ull, __ATOMIC_ACQ_REL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) {
							__hip_atomic_store(&ctl->closing, p.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
							leave = 1u;
						}
					}
				}
				if (uniform_u32(leave)) return 0xFFFFFFFFu;
			}
		}
	}
}

// Register budgets.  Up to 1080p (16-bit tile table): four waves per SIMD = 128 VGPRs requested -- the wave allocates 136-144 with the
// SGPRs it spills on top, three per SIMD in fact -- and a ray's first batches read in groups of 16 samples.  Above 1080p (compact
// index): three waves per SIMD = 168 VGPRs, which has room for a whole 32-sample batch of window reads in flight without a scratch
// access in any loop (tools/scratch_in_loops.py) and for eight compact-index entries per long-ray group: +6 % on the reference's
// 1440p screenshots.  Beside either a SIMD has room for two 128-register waves of the streaming pass (168 + 256 <= 512 < 144 + 384),
// which is also all the LDS beside a service workgroup allows.  (The 168-register build on 1080p frames: 487 k against 511 k for the
// synthetic scene, six interleaved runs on one box -- hence two kernels, each with callees of its own.)
#define SVC_MAX_WAVES 4
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wpass-failed"
template <bool COMPACT>
__device__ __forceinline__ void svc_kernel_body(const Geom &g, const SvcParams &p) {
	extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
	__shared__ uint32_t cull_tab[SMH_CULL_TAB_WORDS];
	__shared__ RayDir s_dirs[SMH_LSD_RAYS];                     // the ray directions, once per launch: no global load in the scan
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	if (p.cull_tab) for (uint32_t i = threadIdx.x; i < SMH_CULL_TAB_WORDS; i += blockDim.x) cull_tab[i] = p.cull_tab[i];
	for (uint32_t i = threadIdx.x; i < SMH_LSD_RAYS; i += blockDim.x) s_dirs[i] = g_ray_table[i];
	if (lane == 0) {
		WShared &w0 = *(WShared *)(smem + wave * p.part_words);
		w0.want_set = 0u; w0.late = 0u;
		if (SVC_WIN_REUSE(COMPACT)) w0.frame_no = 0u;
		const uint32_t owner = blockIdx.x * (blockDim.x >> 6) + wave;
		const bool rem = p.remote != nullptr && !(p.flags & 8u) && owner < 0x10000u;
		w0.rem_r = rem ? (unsigned long long)(uintptr_t)(p.remote + owner) : 0ull;
		w0.rem_store = (unsigned long long)(uintptr_t)(p.remote_store + (size_t)owner * p.remote_store_words);
		w0.rem_ctl = (unsigned long long)(uintptr_t)p.ctl;
		w0.rem_after = p.remote_after; w0.rem_tickets = p.remote_tickets; w0.rem_owner = owner; w0.rem_cap = p.tile_cap;
		w0.rem_open = 0u; w0.rem_gen = 0u; w0.rem_k = 0u; w0.rem_nr = 0u;
		w0.rem_last_div = p.remote_last_div; w0.rem_flags = (p.flags & 16u) ? 1u : 0u;
	}
	__syncthreads();                                            // the only workgroup-wide barrier: from here on every wave is on its own
	uint32_t *part = smem + wave * p.part_words;
	const uint32_t nw = blockDim.x >> 6;
	const bool team = nw > 1u && !(p.flags & 8u);
	if (p.flags & 4u) __builtin_amdgcn_s_setprio(3);            // experiment: the search wave ahead of the streaming waves of its SIMD
	const unsigned long long t_start = __builtin_amdgcn_s_memtime();
	unsigned long long t_busy = 0ull, t_help = 0ull, t_phase[4] = {0ull, 0ull, 0ull, 0ull}, rt_wait = 0ull;
	uint32_t n_items = 0u;
	while (true) {
		// between two frames of its own: a frame of this workgroup that has been at work for a while comes first -- what keeps a
		// batch's slot busy is its slowest frame.  (Measured against popping a waiting frame first and helping only with an
		// empty ring: 435 k against 361 k frames/s at depth 8, 520 k against 460 k at depth 12 -- the old frames are the ones
		// whose slots the host is waiting for.)
		if (team) {
			const uint32_t sib = svc_sibling_in_need(smem, p.part_words, nw, uniform_u32(wave));
			if (sib != 0xFFFFFFFFu) {
				const unsigned long long t_h = __builtin_amdgcn_s_memtime();
				svc_help<COMPACT>((const void *)__builtin_amdgcn_kernarg_segment_ptr(), sib, lds_off(part), lds_off(cull_tab), lds_off(s_dirs));
				t_help += __builtin_amdgcn_s_memtime() - t_h;
				continue;
			}
		}
		uint32_t help_ticket = 0;
		const uint32_t item = svc_pop(p, team ? smem : nullptr, nw, uniform_u32(wave), blockIdx.x == 0u && uniform_u32(wave) == 0u, &help_ticket);
		if (item == 0xFFFFFFFEu) continue;                      // (a sibling asked for help while this wave was waiting for work)
		if (item == 0xFFFFFFFDu) {                              // a frame of another workgroup has asked
			const unsigned long long t_h = __builtin_amdgcn_s_memtime();
			svc_help_remote<COMPACT>((const void *)__builtin_amdgcn_kernarg_segment_ptr(), help_ticket, lds_off(part), lds_off(cull_tab), lds_off(s_dirs));
			t_help += __builtin_amdgcn_s_memtime() - t_h;
			continue;
		}
		if (item == 0xFFFFFFFFu) break;
		const unsigned long long t_item = __builtin_amdgcn_s_memtime(), rt_item = __builtin_amdgcn_s_memrealtime();
		const uint32_t slot = item >> 24, f = item & 0xFFFFFFu;
		// what the streaming side of this submission wrote (mask, aux, scales image, the slot's descriptor) -- by kernels that
		// ran while this one was already resident
		if (!(p.flags & 1u)) {
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
			__builtin_amdgcn_s_dcache_inv();
		}
		const unsigned long long t_acq = __builtin_amdgcn_s_memtime();
		const unsigned long long t_srch = svc_frame<COMPACT>((const void *)__builtin_amdgcn_kernarg_segment_ptr(), slot, f, lds_off(part), lds_off(cull_tab), lds_off(s_dirs));
		const unsigned long long t_rec = __builtin_amdgcn_s_memtime();
		// the record is in memory before the frame is counted off
		if (!(p.flags & 2u)) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
		if (lane == 0) {
			SvcSlot *sl = p.slots + slot;
			const uint32_t n = __hip_atomic_load(&sl->n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), seq = __hip_atomic_load(&sl->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			const unsigned long long t_pub = __hip_atomic_load(&sl->t_pub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), rt_now = __builtin_amdgcn_s_memrealtime();
			rt_wait += rt_item - t_pub;
			__hip_atomic_fetch_sub(&p.ctl->busy, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			if (__hip_atomic_fetch_add(&sl->done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + 1u == n) {
				// the submission's last frame: tell the host (smhv_pipeline_wait polls this word), then count the submission
				__hip_atomic_store(&p.host->done_seq[slot], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
				__hip_atomic_fetch_add(&p.ctl->stat_t_sub, rt_now - t_pub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				__hip_atomic_fetch_add(&p.ctl->stat_t_last, rt_now - rt_item, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				__hip_atomic_fetch_add(&p.ctl->completed, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
			}
		}
		const unsigned long long t_end = __builtin_amdgcn_s_memtime();
		t_busy += t_end - t_item;
		t_phase[0] += t_acq - t_item; t_phase[1] += t_srch - t_acq; t_phase[2] += t_rec - t_srch; t_phase[3] += t_end - t_rec;
		++n_items;
	}
	if (lane == 0) {
		__hip_atomic_fetch_add(&p.ctl->stat_items, n_items, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		__hip_atomic_fetch_add(&p.ctl->stat_waves, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		__hip_atomic_fetch_add(&p.ctl->stat_busy, t_busy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		__hip_atomic_fetch_add(&p.ctl->stat_life, __builtin_amdgcn_s_memtime() - t_start, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		for (int k = 0; k < 4; ++k) __hip_atomic_fetch_add(&p.ctl->stat_phase[k], t_phase[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		__hip_atomic_fetch_add(&p.ctl->stat_help, t_help, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		__hip_atomic_fetch_add(&p.ctl->stat_t_wait, rt_wait, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}
__global__ void __launch_bounds__(64 * SVC_MAX_WAVES) __attribute__((amdgpu_waves_per_eu(4, 4))) k_lsd_service(Geom g, SvcParams p) { svc_kernel_body<false>(g, p); }
__global__ void __launch_bounds__(64 * SVC_MAX_WAVES) __attribute__((amdgpu_waves_per_eu(3, 3))) k_lsd_service_c(Geom g, SvcParams p) { svc_kernel_body<true>(g, p); }
#pragma clang diagnostic pop

// One-shot probe at pipeline creation: the service's life cycle rests on 64-bit system-scope compare-and-swaps and stores into
// mapped host memory (SvcHost::state, done_seq).  Where the platform does not route PCIe atomics (some hosts, VMs,
// passthrough) such a compare-and-swap fails silently and a launch could never close: the pipeline then keeps the
// batch-granular search.  The host puts `expect` into SvcHost::pad[0..1]; the kernel swaps it for `desired` and reports.
__global__ void k_svc_probe(SvcHost *host, unsigned long long expect, unsigned long long desired, uint32_t *ok) {
	unsigned long long *w = (unsigned long long *)&host->pad[0];
	unsigned long long e = expect;
	const bool swapped = __hip_atomic_compare_exchange_strong(w, &e, desired, __ATOMIC_ACQ_REL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	__hip_atomic_store(&host->pad[2], swapped ? 0x600Du : 0xBADu, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
	*ok = swapped ? 1u : 0u;
}

// The last kernel of a submission's streaming side: the slot's descriptor, then its n items.  One workgroup.
__global__ void __launch_bounds__(256) k_svc_publish(SvcCtl *ctl, unsigned long long *ring, SvcSlot *slots, uint32_t slot, Buffers b, uint32_t n, uint32_t seq, uint32_t ring_log2) {
	__shared__ uint32_t s_base;
	if (threadIdx.x == 0) {
		SvcSlot *sl = slots + slot;
		sl->b = b;
		__hip_atomic_store(&sl->n, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		__hip_atomic_store(&sl->seq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		__hip_atomic_store(&sl->done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		__hip_atomic_store(&sl->t_pub, (unsigned long long)__builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		s_base = __hip_atomic_fetch_add(&ctl->reserve, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	__syncthreads();
	const uint32_t base = s_base, mask = (1u << ring_log2) - 1u;
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");          // (thread 0: the descriptor before any item that names the slot)
	for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
		const uint32_t t = base + i;
		__hip_atomic_store(ring + (t & mask), ((unsigned long long)((t >> ring_log2) + 1u) << 32) | (slot << 24) | i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
	__syncthreads();
	if (threadIdx.x == 0) __hip_atomic_fetch_add(&ctl->avail, (int32_t)n, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
