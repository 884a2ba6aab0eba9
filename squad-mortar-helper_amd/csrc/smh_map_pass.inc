// smh_map_pass.inc -- the body of k_map_pass (smh_stream.hip), included once per kernel that runs it: k_map_pass and k_map_pass_luma.
// The including kernel has the parameters (Geom g, Buffers b, uint32_t flags, uint32_t RB), the template parameter TILES and a
// constexpr int GRAYF: 0 = colour, 1 = grey as (l,l,l,255), 2 = grey as a luma plane -- one byte per pixel, b.ui = the plane, row
// pitch ui_pitch / 4, frame stride ui_stride / 4 (smh_kernels.h, "the grey ui_map as a luma plane").  Text, not a function: k_map_pass
// compiles to the code it was before the plane existed, to the instruction.
	const uint32_t f = blockIdx.y;
	if (!b.aux[f].open) return;
	const uint32_t q = threadIdx.x, lane = q & 63u, wave = q >> 6, nwave = blockDim.x >> 6;
	const int r0 = (int)(blockIdx.x * RB);
	const int r1 = min(r0 + (int)RB, (int)g.rh);
	const bool qact = q < g.m_quads;
	uint32_t vmask = 0;
#pragma unroll
	for (int c = 0; c < 4; ++c)
		if ((uint32_t)(4 * q + c - g.m_xoff) < g.rw) vmask |= 1u << c;
	if (!qact) vmask = 0;

	const uint8_t *fp = b.frames + (size_t)f * g.frame_bytes + ((size_t)g.ry * g.W + g.m_ax + 4 * q) * 4;
	uint8_t *uip = GRAYF == 2 ? b.ui + (size_t)f * (g.ui_stride >> 2) + (size_t)q * 4 : b.ui + (size_t)f * g.ui_stride + (size_t)q * 16;
	const size_t row_bytes = (size_t)g.W * 4;

	uint64_t P[4] = {0, 0, 0, 0};
	const int rs = max(r0 - 1, 0), re = min(r1, (int)g.rh - 1);
	const bool do_ui = (flags & MAP_UI) != 0, do_mask = (flags & MAP_MASK) != 0;

	// Software pipeline: the loads of the next four rows are issued before the current four are
	// processed, so they fly under the compute and the stores (vmcnt is in-order: a load issued after
	// the stores would also wait for them).  Inactive lanes re-read quad 0 (no divergent load).
	const uint8_t *lp = qact ? fp : fp - (size_t)q * 16;
	uint4 nx[4];
#pragma unroll
	for (int k = 0; k < 4; ++k) nx[k] = *(const uint4 *)(lp + (size_t)min(rs + k, re) * row_bytes);
	// per-wave hit lists, sized by the launch (640 bytes per wave: 2.5 KB at 1080p, so that several of these workgroups fit
	// into the LDS a k_lsd workgroup of the other pipelined step leaves free on its CU)
	extern __shared__ __attribute__((aligned(16))) uint32_t s_hits[];
	for (int r = rs; r <= re; r += 4) {
		uint4 px[4];
		uint32_t prehits = 0;
#pragma unroll
		for (int k = 0; k < 4; ++k) px[k] = nx[k];
		if (r + 4 <= re) {
#pragma unroll
			for (int k = 0; k < 4; ++k) nx[k] = *(const uint4 *)(lp + (size_t)min(r + 4 + k, re) * row_bytes);
		}
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			const int row = r + k;
			if (row > re) break;
			const uint32_t pv[4] = {px[k].x, px[k].y, px[k].z, px[k].w};
			if (do_ui && row >= r0 && row < r1 && qact) {
				uint32_t ov[4];
#pragma unroll
				for (int c = 0; c < 4; ++c) {
					const uint32_t p = pv[c], bb = p & 255u, gg = (p >> 8) & 255u, rr8 = (p >> 16) & 255u;
					if (GRAYF == 2) ov[c] = luma8(rr8, gg, bb);                          // Bgra::to_luma, the byte alone
					else if (GRAYF) ov[c] = luma8(rr8, gg, bb) * 0x00010101u | 0xFF000000u;   // Bgra::to_luma -> (l,l,l,255)
					else ov[c] = rr8 | (gg << 8) | (bb << 16) | 0xFF000000u;           // (r,g,b,255)
				}
				if constexpr (GRAYF == 2) *(uint32_t *)(uip + (size_t)row * (g.ui_pitch >> 2)) = ov[0] | (ov[1] << 8) | (ov[2] << 16) | (ov[3] << 24);
				else {
					uint4 o;
					o.x = ov[0]; o.y = ov[1]; o.z = ov[2]; o.w = ov[3];
					*(uint4 *)(uip + (size_t)row * g.ui_pitch) = o;
				}
			}
			if (do_mask) {
				// branch-free integer pre-filter; hits of the four rows are collected (bit 4k+c)
				uint32_t pre = 0;
#pragma unroll
				for (int c = 0; c < 4; ++c) pre |= marker_prefilter(pv[c]) ? (1u << c) : 0u;
				prehits |= (pre & vmask) << (4 * k);
			}
		}
		// ---- exact f32 HSV test for the pre-filter hits of this wave, one hit per lane ----
		// A marker line crosses most rows of a band but only a few pixels of each, so testing hits where
		// they sit would run the (long, divergent) exact test several times per row for two or three
		// active lanes.  Instead the hit pixels of the whole wave and of all four rows are compacted into
		// a 64-entry LDS list, every lane tests one of them, and the verdicts are scattered back with
		// LDS atomic ORs.  (This path used to be 40 % of the kernel's time.)
		if (do_mask && __any(prehits != 0u)) {
			uint32_t *hpx = s_hits + wave * 160u;
			uint32_t *hres = hpx + 64;
			unsigned short *hid = (unsigned short *)(hres + 64);
			const uint32_t cnt = (uint32_t)__popc(prehits);
			uint32_t incl = cnt;
			for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o); if (lane >= (uint32_t)o) incl += t; }
			const uint32_t total = __shfl(incl, 63);
			const uint32_t off = incl - cnt;
			hres[lane] = 0u;
			for (uint32_t base = 0; base < total; base += 64u) {
				uint32_t o = off - base;                           // may wrap: compared unsigned below
#pragma unroll
				for (int k = 0; k < 4; ++k) {
					const uint32_t pk[4] = {px[k].x, px[k].y, px[k].z, px[k].w};
#pragma unroll
					for (int c = 0; c < 4; ++c)
						if ((prehits >> (4 * k + c)) & 1u) {
							if (o < 64u) { hpx[o] = pk[c]; hid[o] = (unsigned short)((lane << 4) | (uint32_t)(4 * k + c)); }
							++o;
						}
				}
				__builtin_amdgcn_wave_barrier();
				const uint32_t e = base + lane;
				if (e < total) {
					const uint32_t p = hpx[lane];
					if (marker_exact((p >> 16) & 255u, (p >> 8) & 255u, p & 255u)) {
						const uint32_t id = hid[lane];
						atomicOr(&hres[id >> 4], 1u << (id & 15u));
					}
				}
				__builtin_amdgcn_wave_barrier();
			}
			const uint32_t res = hres[lane];                       // bit 4k+c: pixel c of row r+k is a marker colour
			if (res) {
				const int sh = r - (r0 - 1);
#pragma unroll
				for (int c = 0; c < 4; ++c) {
					uint32_t y = (res >> c) & 0x1111u;                 // rows k = 0..3 at bits 0,4,8,12
					y = (y | (y >> 3) | (y >> 6) | (y >> 9)) & 0xFu;   // -> bits 0..3
					P[c] |= (uint64_t)y << sh;
				}
			}
		}
	}
	if (!do_mask) return;

	// ---- dilation on the column masks ----
	__shared__ uint64_t s_edge_first[16], s_edge_last[16];
	if (lane == 0) s_edge_first[wave] = P[0];
	if (lane == 63) s_edge_last[wave] = P[3];
	__syncthreads();
	uint64_t left = __shfl_up(P[3], 1), right = __shfl_down(P[0], 1);
	if (lane == 0) left = wave > 0 ? s_edge_last[wave - 1] : 0ull;
	if (lane == 63) right = wave + 1 < nwave ? s_edge_first[wave + 1] : 0ull;
	const int nrows = r1 - r0;
	const uint64_t rowmask = ((nrows >= 63 ? ~0ull : ((1ull << nrows) - 1ull)) << 1);   // bits 1..nrows
	uint64_t D[4];
#define SMH_VERT(p) ((p) | ((p) << 1) | ((p) >> 1))
	D[0] = SMH_VERT(P[0]) | left | P[1];
	D[1] = SMH_VERT(P[1]) | P[0] | P[2];
	D[2] = SMH_VERT(P[2]) | P[1] | P[3];
	D[3] = SMH_VERT(P[3]) | P[2] | right;
#undef SMH_VERT
#pragma unroll
	for (int c = 0; c < 4; ++c) D[c] = ((vmask >> c) & 1u) ? (D[c] & rowmask) : 0ull;

	// ---- outputs: bit-packed rows, and with MAP_BYTES (the per-call path, which hands the mask straight to the host) the u8 mask
	// rows; a batch run leaves those to k_mask_expand (smh_misc.hip) ----
	const bool do_bytes = (flags & MAP_BYTES) != 0;            // (uniform: a kernel argument)
	const uint32_t quads_padded = (g.m_quads + 15u) & ~15u;
	const uint64_t any = D[0] | D[1] | D[2] | D[3];
	const uint64_t lanes_set = __ballot(any != 0ull);
	// the tile-major mask and its occupancy bytes (TILES: bands of whole tile rows, launch_map_pass; a launch without them runs the
	// instantiation that has no trace of this)
	uint32_t occ7 = 0;
	if constexpr (TILES) {
		const uint32_t ntr = ((uint32_t)nrows + 7u) >> 3, op = occ_pitch(g);
		uint8_t *occp = b.occ + (size_t)f * occ_stride(g) + (size_t)((uint32_t)r0 >> 3) * op + wave;
		if (lanes_set) occ7 = tile_occupancy(any >> 1, lane, ntr, occp, op);
		else if (lane < ntr) occp[(size_t)lane * op] = 0;
		if (blockIdx.x == 0 && q == 0) b.aux[f].tiles = 1u;           // (k_button cleared it: this frame's tile-major mask is being written)
	}
	if (q < quads_padded) {
		uint8_t *mp = b.mask + (size_t)f * g.mask_stride + (size_t)q * 4;
		uint32_t *bp = b.bits + (size_t)f * g.bits_stride_w + (q >> 3);
		uint32_t *tp = nullptr;
		if constexpr (TILES) tp = b.tiled + (size_t)f * tiled_stride_w(g) + ((size_t)((uint32_t)r0 >> 3) * g.bits_pitch_w + (q >> 3)) * 8u;
		for (int row = r0; row < r1; ++row) {
			const int bit = row - r0 + 1;
			const uint32_t nib = (uint32_t)((D[0] >> bit) & 1ull) | ((uint32_t)((D[1] >> bit) & 1ull) << 1) |
			                     ((uint32_t)((D[2] >> bit) & 1ull) << 2) | ((uint32_t)((D[3] >> bit) & 1ull) << 3);
			if (do_bytes) *(uint32_t *)(mp + (size_t)row * g.mask_pitch) = ((nib * 0x00204081u) & 0x01010101u) * 0xFFu;
			// gather 8 lanes' nibbles into one dword of the bit-packed row (lane l supplies bits 4(l%8)..)
			uint32_t v = nib;
			v |= __shfl_down(v, 1) << 4;
			v |= __shfl_down(v, 2) << 8;
			v |= __shfl_down(v, 4) << 16;
			if ((lane & 7u) == 0) bp[(size_t)row * g.bits_pitch_w] = v;
			if constexpr (TILES) {
				const uint32_t i = (uint32_t)(row - r0);
				if ((occ7 >> (i >> 3)) & 1u) tp[(size_t)(i >> 3) * g.bits_pitch_w * 8u + (i & 7u)] = v;    // (occ7 is 0 outside the lanes 8 j)
			}
		}
	}
	// ---- bounding box + population count of the set bits (drives the LDS window of k_lsd) ----
	if (lanes_set) {
		const uint64_t rows_set = wave_or64(any);
		const uint32_t cnt = wave_sum32(__popcll(D[0]) + __popcll(D[1]) + __popcll(D[2]) + __popcll(D[3]));
		if (lane == 0) {
			FrameAux *a = &b.aux[f];
			atomicMin(&a->y_min, (uint32_t)(r0 - 1 + __builtin_ctzll(rows_set)));
			atomicMax(&a->y_max, (uint32_t)(r0 - 1 + 63 - __builtin_clzll(rows_set)));
			atomicMin(&a->w_min, (wave * 64u + (uint32_t)__builtin_ctzll(lanes_set)) >> 3);
			atomicMax(&a->w_max, (wave * 64u + 63u - (uint32_t)__builtin_clzll(lanes_set)) >> 3);
			atomicAdd(&a->n_mask_px, cnt);
		}
	}
