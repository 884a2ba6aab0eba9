// smh_scalelabels.hip -- scale labels (smh_vision_hip.h, "scale labels"): the words of the ocr_preprocess plane, their boxes, the
// scale bar under each and the glyph crops.  One workgroup of 16 waves per frame; everything between the plane and the record
// lives in LDS.  Every value is an integer (find_scale_width, shared with the record kernels, forms max_scale_y_offset and the
// ratio it is not asked for in f64, as it does there).
//   1. runs      a wave takes a row at a time: two 16-byte loads per lane cover the padded row (at most 2048 bytes), every lane
//                makes the foreground bits of its 16 columns, and with its neighbours' bits beside them (g + 1 <= 14 < 16: one lane
//                to either side is enough, the second half of the row hangs on the first by lanes 63 | 0) a run starts at a
//                foreground bit with no foreground bit in the g + 1 columns before it and ends at one with none in the g + 1 after
//                it.  The k-th start and the k-th end of a row are one run: a wave-wide prefix sum over the lanes' counts gives each
//                lane its place, one LDS add per row the row's place in the list.  Byte-per-lane ballots would take eleven
//                dependent loads for a 657-column row where this takes one.
//   2. words     union-find over the run list: a run is united with the runs of the row above that it touches (they are sorted by
//                l: a binary search finds the first, the rest follow).  The smaller index becomes the parent, by compare-and-swap
//                on the root; finds halve their paths.
//   3. boxes     every run folds its extent into its root's box with LDS atomics.
//   4. bars      the roots whose boxes pass the size limits are compacted into a candidate list; the waves take them in turn
//                through find_scale_width on S0.
//   5. output    a proposal's rank is the number of proposals that sort before it; ranks below eight write their records, and the
//                workgroup copies their crops, a dword per thread and cell.
#include <atomic>
#include <cmath>

#include "smh_record.inc"

namespace smh {

#define SL_THREADS 1024u
#define SL_WAVES (SL_THREADS / 64u)
#define SL_PER_THREAD (SMHV_LABEL_MAX_RUNS / SL_THREADS)
// LDS (bytes): the runs' l, r, y (u16 each); parent; the boxes' four sides (u32: atomics); the rows' first run and run count (u16);
// counters and the selected boxes.  After the words are made the run arrays are free: l holds the candidate list, r the proposal
// list, y the candidates' bar rows, and parent the candidates' bar ends.
#define SL_OFF_L 0u
#define SL_OFF_R (SL_OFF_L + 2u * SMHV_LABEL_MAX_RUNS)
#define SL_OFF_Y (SL_OFF_R + 2u * SMHV_LABEL_MAX_RUNS)
#define SL_OFF_PARENT (SL_OFF_Y + 2u * SMHV_LABEL_MAX_RUNS)
#define SL_OFF_BOX (SL_OFF_PARENT + 4u * SMHV_LABEL_MAX_RUNS)
#define SL_OFF_ROW (SL_OFF_BOX + 16u * SMHV_LABEL_MAX_RUNS)
#define SL_OFF_MISC (SL_OFF_ROW + 4u * SMH_SL_MAX_DIM)
#define SL_LDS_BYTES (SL_OFF_MISC + 256u)
static_assert(SL_OFF_MISC % 16u == 0u, "LDS carve");
enum : uint32_t { SL_N_RUNS = 0, SL_N_WORDS, SL_N_CAND, SL_N_PROP, SL_SEL = 8 };   // words of the misc block; SL_SEL: 8 boxes of 4

// the foreground bits of 16 plane bytes (bit i: byte i != 255)
__device__ __forceinline__ uint32_t sl_fg16(const uint4 v) {
	const uint32_t w[4] = {v.x, v.y, v.z, v.w};
	uint32_t m = 0;
#pragma unroll
	for (uint32_t k = 0; k < 4u; ++k)
#pragma unroll
		for (uint32_t c = 0; c < 4u; ++c) m |= (((w[k] >> (8u * c)) & 255u) != 255u ? 1u : 0u) << (4u * k + c);
	return m;
}

// bits [lo, hi) of a 16-bit field that starts at column `base`
__device__ __forceinline__ uint32_t sl_range16(uint32_t base, uint32_t lo, uint32_t hi) {
	uint32_t m = 0;
#pragma unroll
	for (uint32_t i = 0; i < 16u; ++i) m |= (base + i >= lo && base + i < hi ? 1u : 0u) << i;
	return m;
}

__device__ __forceinline__ uint32_t sl_find(volatile uint32_t *parent, uint32_t x) {
	for (;;) {
		const uint32_t p = parent[x];
		if (p == x) return x;
		const uint32_t gp = parent[p];
		if (gp != p) parent[x] = gp;                          // (x is no root and never becomes one again: any ancestor will do)
		x = gp;
	}
}

__device__ __forceinline__ void sl_unite(uint32_t *parent, uint32_t a, uint32_t b) {
	for (;;) {
		a = sl_find(parent, a);
		b = sl_find(parent, b);
		if (a == b) return;
		if (a > b) { const uint32_t t = a; a = b; b = t; }
		if (atomicCAS(&parent[b], b, a) == b) return;        // (b was still a root: it hangs on the smaller index now)
	}
}

__global__ void __launch_bounds__(SL_THREADS) k_scale_labels(ScaleLabelsRun r) {
	extern __shared__ __attribute__((aligned(16))) uint8_t sl_lds[];
	uint16_t *run_l = (uint16_t *)(sl_lds + SL_OFF_L), *run_r = (uint16_t *)(sl_lds + SL_OFF_R), *run_y = (uint16_t *)(sl_lds + SL_OFF_Y);
	uint32_t *parent = (uint32_t *)(sl_lds + SL_OFF_PARENT);
	uint32_t *box_l = (uint32_t *)(sl_lds + SL_OFF_BOX), *box_t = box_l + SMHV_LABEL_MAX_RUNS, *box_r = box_t + SMHV_LABEL_MAX_RUNS, *box_b = box_r + SMHV_LABEL_MAX_RUNS;
	uint16_t *row_off = (uint16_t *)(sl_lds + SL_OFF_ROW), *row_cnt = row_off + SMH_SL_MAX_DIM;
	uint32_t *misc = (uint32_t *)(sl_lds + SL_OFF_MISC);
	uint16_t *cand = run_l, *prop = run_r, *bar_y = run_y;
	uint32_t *bar_lr = parent;

	const uint32_t f = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	uint32_t *out_w = (uint32_t *)(r.out + f);
	constexpr uint32_t OUT_WORDS = sizeof(smhv_scale_label_frame) / 4u;
	if (!r.aux[f].open) {                                     // a closed frame: a record of zeros
		if (tid < OUT_WORDS) out_w[tid] = 0u;
		return;
	}
	if (tid < 64u) misc[tid] = 0u;
	__syncthreads();

	// ---- 1. runs ----
	const uint8_t *P = r.ocr + (size_t)f * r.stride;
	const uint32_t colA = lane * 16u, colB = 1024u + lane * 16u;   // plane bytes of this lane; pixel x sits at byte q_xoff + x
	const bool inA = colA < r.pitch, inB = colB < r.pitch;    // (the pitch is a multiple of 64: a lane's 16 bytes are inside or outside)
	const uint32_t validA = sl_range16(colA, r.q_xoff, r.q_xoff + r.qw), validB = sl_range16(colB, r.q_xoff, r.q_xoff + r.qw);
	const uint4 none = make_uint4(~0u, ~0u, ~0u, ~0u);
	uint4 na = none, nb = none;
	if (wave < r.qh) {
		if (inA) na = *(const uint4 *)(P + (size_t)wave * r.pitch + colA);
		if (inB) nb = *(const uint4 *)(P + (size_t)wave * r.pitch + colB);
	}
	for (uint32_t y = wave; y < r.qh; y += SL_WAVES) {         // wave-uniform
		const uint4 a = na, b = nb;
		if (y + SL_WAVES < r.qh) {                            // the next row's bytes fly under this row's work
			if (inA) na = *(const uint4 *)(P + (size_t)(y + SL_WAVES) * r.pitch + colA);
			if (inB) nb = *(const uint4 *)(P + (size_t)(y + SL_WAVES) * r.pitch + colB);
		}
		const uint32_t mA = sl_fg16(a) & validA, mB = sl_fg16(b) & validB;
		const uint32_t upA = __shfl_up(mA, 1), dnA = __shfl_down(mA, 1), upB = __shfl_up(mB, 1), dnB = __shfl_down(mB, 1);
		const uint32_t a63 = __shfl(mA, 63), b0 = __shfl(mB, 0);
		const uint64_t wA = (uint64_t)(lane ? upA : 0u) | ((uint64_t)mA << 16) | ((uint64_t)(lane < 63u ? dnA : b0) << 32);
		const uint64_t wB = (uint64_t)(lane ? upB : a63) | ((uint64_t)mB << 16) | ((uint64_t)(lane < 63u ? dnB : 0u) << 32);
		uint64_t befA = 0, aftA = 0, befB = 0, aftB = 0;
		for (uint32_t k = 1; k <= r.gap + 1u; ++k) { befA |= wA << k; aftA |= wA >> k; befB |= wB << k; aftB |= wB >> k; }
		uint32_t sA = mA & ~(uint32_t)(befA >> 16) & 0xFFFFu, eA = mA & ~(uint32_t)(aftA >> 16) & 0xFFFFu;
		uint32_t sB = mB & ~(uint32_t)(befB >> 16) & 0xFFFFu, eB = mB & ~(uint32_t)(aftB >> 16) & 0xFFFFu;
		// the lanes' places: an inclusive prefix sum of the four counts, 16 bits each (a row has at most 1024 runs)
		const uint64_t mine = (uint64_t)__popc(sA) | ((uint64_t)__popc(eA) << 16) | ((uint64_t)__popc(sB) << 32) | ((uint64_t)__popc(eB) << 48);
		uint64_t inc = mine;
#pragma unroll
		for (uint32_t o = 1; o < 64u; o <<= 1) {
			const uint64_t t = __shfl_up(inc, o);
			if (lane >= o) inc += t;
		}
		const uint64_t tot = __shfl(inc, 63), exc = inc - mine;
		const uint32_t totA = (uint32_t)tot & 0xFFFFu, totAe = (uint32_t)(tot >> 16) & 0xFFFFu, total = totA + ((uint32_t)(tot >> 32) & 0xFFFFu);
		uint32_t base = 0;
		if (lane == 0u) {
			if (total) base = atomicAdd(&misc[SL_N_RUNS], total);
			row_off[y] = (uint16_t)min(base, SMHV_LABEL_MAX_RUNS);
			row_cnt[y] = (uint16_t)total;
		}
		base = __shfl(base, 0);
		uint32_t is = base + ((uint32_t)exc & 0xFFFFu), ie = base + ((uint32_t)(exc >> 16) & 0xFFFFu);
		for (; sA; sA &= sA - 1u, ++is)
			if (is < SMHV_LABEL_MAX_RUNS) { run_l[is] = (uint16_t)(colA + (uint32_t)__builtin_ctz(sA) - r.q_xoff); run_y[is] = (uint16_t)y; }
		for (; eA; eA &= eA - 1u, ++ie)
			if (ie < SMHV_LABEL_MAX_RUNS) run_r[ie] = (uint16_t)(colA + (uint32_t)__builtin_ctz(eA) - r.q_xoff);
		is = base + totA + ((uint32_t)(exc >> 32) & 0xFFFFu); ie = base + totAe + ((uint32_t)(exc >> 48) & 0xFFFFu);
		for (; sB; sB &= sB - 1u, ++is)
			if (is < SMHV_LABEL_MAX_RUNS) { run_l[is] = (uint16_t)(colB + (uint32_t)__builtin_ctz(sB) - r.q_xoff); run_y[is] = (uint16_t)y; }
		for (; eB; eB &= eB - 1u, ++ie)
			if (ie < SMHV_LABEL_MAX_RUNS) run_r[ie] = (uint16_t)(colB + (uint32_t)__builtin_ctz(eB) - r.q_xoff);
	}
	__syncthreads();
	const uint32_t nr = misc[SL_N_RUNS];
	if (nr > SMHV_LABEL_MAX_RUNS) {                           // (uniform) the list is not whole: no words, no proposals
		if (tid < OUT_WORDS) out_w[tid] = tid == 3u ? nr : (tid == 4u ? SMHV_LABELS_RUNS_OVERFLOW : 0u);
		return;
	}

	// ---- 2. words ----
	for (uint32_t i = tid; i < nr; i += SL_THREADS) {
		const uint32_t y = run_y[i];
		parent[i] = i;
		box_l[i] = run_l[i]; box_r[i] = (uint32_t)run_r[i] + 1u; box_t[i] = y; box_b[i] = y + 1u;
	}
	__syncthreads();
	for (uint32_t i = tid; i < nr; i += SL_THREADS) {
		const uint32_t y = run_y[i];
		if (y == 0u) continue;
		const uint32_t l = run_l[i], rr = run_r[i], off = row_off[y - 1u], end = off + row_cnt[y - 1u];
		uint32_t lo = off, hi = end;                          // the first run of the row above with r + 1 >= l
		while (lo < hi) {
			const uint32_t mid = (lo + hi) >> 1;
			if ((uint32_t)run_r[mid] + 1u >= l) hi = mid; else lo = mid + 1u;
		}
		for (uint32_t j = lo; j < end && (uint32_t)run_l[j] <= rr + 1u; ++j) sl_unite(parent, i, j);
	}
	__syncthreads();

	// ---- 3. boxes; 4. candidates (no store to parent from here on: parent[i] == i is "a root") ----
#pragma unroll
	for (uint32_t k = 0; k < SL_PER_THREAD; ++k) {
		const uint32_t i = tid + k * SL_THREADS;
		if (i < nr) {
			uint32_t root = i;
			for (uint32_t p = parent[root]; p != root; p = parent[root]) root = p;
			if (root != i) {
				const uint32_t y = run_y[i];
				atomicMin(&box_l[root], (uint32_t)run_l[i]); atomicMax(&box_r[root], (uint32_t)run_r[i] + 1u);
				atomicMin(&box_t[root], y); atomicMax(&box_b[root], y + 1u);
			}
		}
	}
	__syncthreads();
	bool is_cand[SL_PER_THREAD];
#pragma unroll
	for (uint32_t k = 0; k < SL_PER_THREAD; ++k) {
		const uint32_t i = tid + k * SL_THREADS;
		const bool root = i < nr && parent[i] == i;
		const uint32_t bw = root ? box_r[i] - box_l[i] : 0u, bh = root ? box_b[i] - box_t[i] : 0u;
		is_cand[k] = root && bw >= 3u && bw <= SMHV_LABEL_CROP_W && bh >= 3u && bh <= SMHV_LABEL_CROP_H;
		const uint32_t words = (uint32_t)__popcll(__ballot(root));
		if (lane == 0u && words) atomicAdd(&misc[SL_N_WORDS], words);
	}
	__syncthreads();                                           // the run arrays are free: the candidate list goes into l's place
#pragma unroll
	for (uint32_t k = 0; k < SL_PER_THREAD; ++k) {
		const uint64_t m = __ballot(is_cand[k]);
		uint32_t base = 0;
		if (lane == 0u && m) base = atomicAdd(&misc[SL_N_CAND], (uint32_t)__popcll(m));
		base = __shfl(base, 0);
		if (is_cand[k]) cand[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)(tid + k * SL_THREADS);
	}
	__syncthreads();

	// ---- 4. bars: a wave per candidate (find_scale_width's verdicts are ballots: every lane holds the same) ----
	const uint32_t nc = misc[SL_N_CAND];
	const uint8_t *S0 = r.s0 + (size_t)f * r.stride + r.q_xoff;
	for (uint32_t c = wave; c < nc; c += SL_WAVES) {
		const uint32_t root = cand[c];
		const uint32_t ax = (box_l[root] + box_r[root]) >> 1, ay = box_b[root];
		double ratio = 0.0;
		uint32_t bar[3] = {0, 0, 0};
		const bool ok = find_scale_width(S0, r.pitch, r.qw, r.qh, 1u, ax, ay, &ratio, bar);
		if (lane == 0u) {
			bar_lr[c] = (ok && bar[2] > bar[0]) ? (bar[0] | (bar[2] << 16)) : 0xFFFFFFFFu;   // (a wrapped width is no proposal)
			bar_y[c] = (uint16_t)bar[1];
		}
	}
	__syncthreads();
	for (uint32_t c = tid; c < nc; c += SL_THREADS)
		if (bar_lr[c] != 0xFFFFFFFFu) prop[atomicAdd(&misc[SL_N_PROP], 1u)] = (uint16_t)c;
	__syncthreads();

	// ---- 5. output ----
	const uint32_t np = misc[SL_N_PROP], n = min(np, SMHV_MAX_SCALE_LABELS);
	for (uint32_t p = tid; p < np; p += SL_THREADS) {
		const uint32_t c = prop[p], root = cand[c];
		const uint32_t l = box_l[root], t = box_t[root], rr = box_r[root], bt = box_b[root];
		const uint64_t key = ((uint64_t)t << 48) | ((uint64_t)l << 32) | ((uint64_t)rr << 16) | (uint64_t)bt;
		uint32_t rank = 0;
		for (uint32_t q = 0; q < np; ++q) {
			const uint32_t rq = cand[prop[q]];
			const uint64_t kq = ((uint64_t)box_t[rq] << 48) | ((uint64_t)box_l[rq] << 32) | ((uint64_t)box_r[rq] << 16) | (uint64_t)box_b[rq];
			rank += (kq < key || (kq == key && q < p)) ? 1u : 0u;
		}
		if (rank < SMHV_MAX_SCALE_LABELS) {
			const uint32_t lr = bar_lr[c];
			smhv_scale_label lb;
			lb.left = l; lb.top = t; lb.right = rr; lb.bottom = bt;
			lb.bar_left = lr & 0xFFFFu; lb.bar_y = bar_y[c]; lb.bar_right = lr >> 16; lb.width = lb.bar_right - lb.bar_left;
			r.out[f].label[rank] = lb;
			uint32_t *sel = misc + SL_SEL + 4u * rank;
			sel[0] = l; sel[1] = t; sel[2] = rr; sel[3] = bt;
		}
	}
	if (tid < 8u) out_w[tid] = tid == 0u ? n : (tid == 1u ? np : (tid == 2u ? misc[SL_N_WORDS] : (tid == 3u ? nr : 0u)));
	else if (tid < OUT_WORDS && (tid - 8u) / 8u >= n) out_w[tid] = 0u;   // the records past n
	__syncthreads();
	// the crops: cell s, row tid / 32, bytes 4 (tid % 32) .. + 3
	uint8_t *cells = r.crops + (size_t)f * SMHV_LABEL_FRAME_CROP_BYTES;
	const uint32_t cy = tid >> 5, cx = (tid & 31u) * 4u;
	for (uint32_t s = 0; s < n; ++s) {
		const uint32_t *sel = misc + SL_SEL + 4u * s;
		const uint32_t l = sel[0], t = sel[1], rr = sel[2], bt = sel[3];
		uint32_t word = 0;
#pragma unroll
		for (uint32_t k = 0; k < 4u; ++k) {
			const uint32_t x = l + cx + k, y = t + cy;
			const uint32_t v = (x < rr && y < bt) ? P[(size_t)y * r.pitch + r.q_xoff + x] : 255u;
			word |= v << (8u * k);
		}
		*(uint32_t *)(cells + (size_t)s * SMHV_LABEL_CROP_BYTES + (size_t)tid * 4u) = word;
	}
}

uint32_t scale_labels_gap(uint32_t qw) {
	const double g = std::round((4.0 / 640.0) * (double)qw);
	return g < 1.0 ? 1u : (uint32_t)g;
}

hipError_t launch_scale_labels(const ScaleLabelsRun &r, uint32_t n, hipStream_t s) {
	static_assert(SL_THREADS * 4u == SMHV_LABEL_CROP_BYTES, "a dword per thread and cell");
	static_assert(sizeof(smhv_scale_label_frame) == 288u && sizeof(smhv_scale_label) == 32u, "record layout");
	if (n == 0u || !r.aux || !r.ocr || !r.s0 || !r.out || !r.crops || r.qw == 0u || r.qh == 0u || r.qh > SMH_SL_MAX_DIM || r.pitch > SMH_SL_MAX_DIM ||
	    (r.pitch & 63u) != 0u || r.q_xoff + r.qw > r.pitch || r.gap == 0u || r.gap > 13u)
		return hipErrorInvalidValue;
	static std::atomic<uint64_t> attr_set{0};                 // per device: the kernel may take more than the default 64 KB of LDS
	int dev = 0;
	hipError_t e = hipGetDevice(&dev);
	if (e != hipSuccess) return e;
	if (dev < 0 || dev >= 64 || !((attr_set.load(std::memory_order_acquire) >> dev) & 1ull)) {
		e = hipFuncSetAttribute((const void *)k_scale_labels, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SL_LDS_BYTES);
		if (e != hipSuccess) return e;
		if (dev >= 0 && dev < 64) attr_set.fetch_or(1ull << dev, std::memory_order_release);
	}
	hipLaunchKernelGGL(k_scale_labels, dim3(n), dim3(SL_THREADS), SL_LDS_BYTES, s, r);
	return hipGetLastError();
}

}  // namespace smh
