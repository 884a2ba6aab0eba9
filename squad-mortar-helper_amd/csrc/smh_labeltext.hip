// smh_labeltext.hip -- scale labels: text (smh_vision_hip.h, "scale labels: text"; the rule's one text is smh_glyph_rule.h).  One
// workgroup of eight waves per frame, wave w on label w; a few thousand popcounts per label: the kernel is shaped by latency, so
// every phase is one round of LDS traffic and the phases are separated by workgroup barriers that every wave reaches.
//   0. stage    the atlas (4368 bytes) and a record of zeros into LDS.
//   1. bits     a wave loads its 4 KB cell with four 16-byte loads per lane (load j of lane L: row 8 j + L / 8, columns 16 (L % 8) ..),
//               masks the foreground bits by the label's box and leaves 32 row masks of 128 bits in LDS.
//   2. glyphs   lane y < 32 holds row y; the OR over the lanes is the column occupancy, its runs are the glyphs (every lane walks
//               them: the values are uniform).  A glyph's rows are a shift and a mask of the lanes' rows, its first and last row a
//               ballot; the tight bitmap goes to LDS, 32 words a glyph.
//   3. match    per glyph the lanes stride over the (template, shift) pairs -- at most 288, five a lane, kept in registers -- and the
//               wave takes the least key (distance << 8 | template) by shuffles, then the least key among the other codes.  Lane 0
//               writes the glyph's character and numbers into the record in LDS, and after the last glyph the text's meters.
//   4. frame    thread 0 applies the anchors' rule to the eight meters.
//   5. output   the record and the anchors leave LDS a dword per thread.
// No scratch: nothing is indexed by a run-time value but LDS and global memory.
#include "smh_kernels.h"
#include "smh_glyph_rule.h"

namespace smh {

#define LT_THREADS 512u
#define LT_WAVES (LT_THREADS / 64u)
#define LT_PAIRS_PER_LANE 5u
static_assert(LT_WAVES == SMHV_MAX_SCALE_LABELS, "a wave per label");
static_assert(SMHV_ATLAS_MAX_TEMPLATES * 9u <= LT_PAIRS_PER_LANE * 64u, "a glyph's pairs fit the lanes' registers");
static_assert(SMHV_LABEL_CROP_BYTES == 4u * 64u * 16u && SMHV_LABEL_CROP_W == 128u && SMHV_LABEL_CROP_H == 32u, "four 16-byte loads per lane cover a cell");

struct LtWave {
	uint32_t rows[32][4];                // the cell's foreground bits
	uint32_t glyph[SMHV_LABEL_MAX_GLYPHS][32];
	uint32_t gmeta[SMHV_LABEL_MAX_GLYPHS];   // w | h << 8 (h = 0: wider than 32 columns)
};
struct LtLds {
	smhv_label_text_frame rec;
	GlyphAtlas atlas;
	LtWave wave[LT_WAVES];
	uint32_t meters[SMHV_MAX_SCALE_LABELS];
};
static_assert(sizeof(LtLds) <= 32768u, "LDS");

// the foreground bits of 16 cell bytes (bit i: byte i != 255)
__device__ __forceinline__ uint32_t lt_fg16(const uint4 v) {
	const uint32_t w[4] = {v.x, v.y, v.z, v.w};
	uint32_t m = 0;
#pragma unroll
	for (uint32_t k = 0; k < 4u; ++k)
#pragma unroll
		for (uint32_t c = 0; c < 4u; ++c) m |= (((w[k] >> (8u * c)) & 255u) != 255u ? 1u : 0u) << (4u * k + c);
	return m;
}

__device__ __forceinline__ uint32_t lt_wave_min(uint32_t v) {
#pragma unroll
	for (uint32_t o = 1; o < 64u; o <<= 1) v = min(v, (uint32_t)__shfl_xor((int)v, (int)o));
	return v;
}

__device__ __forceinline__ uint64_t lt_wave_or(uint64_t v) {
#pragma unroll
	for (uint32_t o = 1; o < 64u; o <<= 1) v |= (uint64_t)__shfl_xor((unsigned long long)v, (int)o);
	return v;
}

__global__ void __launch_bounds__(LT_THREADS) k_label_text(LabelTextRun r) {
	__shared__ LtLds S;
	const uint32_t f = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const smhv_scale_label_frame *F = r.labels + f;
	const uint32_t n = min(F->n, (uint32_t)SMHV_MAX_SCALE_LABELS);   // (a closed frame, a frame whose run list overflowed: 0)
	const bool mine = wave < n;                                // wave-uniform: the cells i >= n are never read
	LtWave &W = S.wave[wave];
	smhv_label_text_entry &T = S.rec.label[wave];

	// ---- 0. stage; 1. bits ----
	uint4 v[4];
	uint32_t bw = 0, bh = 0;
	if (mine) {
		const uint8_t *cell = r.crops + (size_t)f * SMHV_LABEL_FRAME_CROP_BYTES + (size_t)wave * SMHV_LABEL_CROP_BYTES;
#pragma unroll
		for (uint32_t j = 0; j < 4u; ++j) v[j] = *(const uint4 *)(cell + (size_t)(j * 64u + lane) * 16u);
		bw = min(F->label[wave].right - F->label[wave].left, (uint32_t)SMHV_LABEL_CROP_W);
		bh = min(F->label[wave].bottom - F->label[wave].top, (uint32_t)SMHV_LABEL_CROP_H);
	}
	{
		uint32_t *dst = (uint32_t *)&S.atlas;
		const uint32_t *src = (const uint32_t *)r.atlas;
		for (uint32_t i = tid; i < sizeof(GlyphAtlas) / 4u; i += LT_THREADS) dst[i] = src[i];
		uint32_t *rec = (uint32_t *)&S.rec;
		for (uint32_t i = tid; i < sizeof(smhv_label_text_frame) / 4u; i += LT_THREADS) rec[i] = 0u;
		if (tid < SMHV_MAX_SCALE_LABELS) S.meters[tid] = 0u;
	}
	if (mine) {
		uint16_t *rows16 = (uint16_t *)W.rows;                 // (little-endian: chunks 2 k and 2 k + 1 are word k of a row)
#pragma unroll
		for (uint32_t j = 0; j < 4u; ++j) {
			const uint32_t idx = j * 64u + lane, row = idx >> 3, col = (idx & 7u) * 16u;
			const uint32_t valid = (row < bh && bw > col) ? (bw - col >= 16u ? 0xFFFFu : ((1u << (bw - col)) - 1u)) : 0u;
			rows16[idx] = (uint16_t)(lt_fg16(v[j]) & valid);
		}
	}
	__syncthreads();

	// ---- 2. glyphs ----
	uint32_t ng = 0;
	if (mine) {
		uint64_t lo = 0, hi = 0;
		if (lane < 32u) {
			lo = (uint64_t)W.rows[lane][0] | ((uint64_t)W.rows[lane][1] << 32);
			hi = (uint64_t)W.rows[lane][2] | ((uint64_t)W.rows[lane][3] << 32);
		}
		const uint64_t olo = lt_wave_or(lo), ohi = lt_wave_or(hi);
		uint32_t l = 0, rr = 0;
		for (uint32_t from = 0; glyph_next_run(olo, ohi, from, &l, &rr); from = rr + 1u) {   // uniform
			if (ng < SMHV_LABEL_MAX_GLYPHS) {
				const uint32_t gw = rr - l + 1u;
				uint32_t gh = 0;
				if (gw <= 32u) {
					const uint32_t word = lane < 32u ? glyph_row_bits(lo, hi, l, gw) : 0u;
					const uint64_t rows = __ballot(word != 0u);      // (a run of non-empty columns has a non-empty row)
					const uint32_t top = (uint32_t)__builtin_ctzll(rows), bot = 63u - (uint32_t)__builtin_clzll(rows);
					gh = bot - top + 1u;
					const uint32_t moved = (uint32_t)__shfl((int)word, (int)((lane + top) & 63u));
					if (lane < 32u) W.glyph[ng][lane] = lane < gh ? moved : 0u;
				}
				if (lane == 0u) W.gmeta[ng] = gw | (gh << 8);
			}
			++ng;
		}
		if (lane == 0u) {
			T.n_glyphs = ng;
			T.flags = ng > SMHV_LABEL_MAX_GLYPHS ? SMHV_LABEL_TEXT_TOO_MANY : 0u;
		}
	}
	__syncthreads();

	// ---- 3. match ----
	if (mine && ng <= SMHV_LABEL_MAX_GLYPHS) {
		const uint32_t nt = min(S.atlas.n, (uint32_t)SMHV_ATLAS_MAX_TEMPLATES), pairs = nt * 9u;
		for (uint32_t k = 0; k < ng; ++k) {
			const uint32_t meta = W.gmeta[k], gh = meta >> 8;
			uint32_t ch = '?', best = SMH_GLYPH_NONE, second = SMH_GLYPH_NONE, tm = SMH_GLYPH_NO_TMPL;
			if (gh) {                                              // (wave-uniform)
				uint32_t key[LT_PAIRS_PER_LANE], least = 0xFFFFFFFFu;
#pragma unroll
				for (uint32_t i = 0; i < LT_PAIRS_PER_LANE; ++i) {
					const uint32_t p = lane + 64u * i;
					key[i] = 0xFFFFFFFFu;
					if (p < pairs) {
						const uint32_t t = p / 9u, s = p - 9u * t;
						key[i] = glyph_key(glyph_shift_distance(W.glyph[k], gh, S.atlas.rows[t], glyph_meta_h(S.atlas.meta[t]), glyph_shift_dx(s), glyph_shift_dy(s)), t);
					}
					least = min(least, key[i]);
				}
				const uint32_t win = lt_wave_min(least), wt = win & 255u, wcode = glyph_meta_code(S.atlas.meta[wt]);
				least = 0xFFFFFFFFu;
#pragma unroll
				for (uint32_t i = 0; i < LT_PAIRS_PER_LANE; ++i)
					if (key[i] != 0xFFFFFFFFu && glyph_meta_code(S.atlas.meta[key[i] & 255u]) != wcode) least = min(least, key[i]);
				const uint32_t sec = lt_wave_min(least);
				best = win >> 8; tm = wt;
				second = sec == 0xFFFFFFFFu ? SMH_GLYPH_NONE : sec >> 8;
				if (glyph_accept(best, S.atlas.fg[wt], S.atlas.accept_num, S.atlas.accept_den)) ch = wcode;
			}
			if (lane == 0u) { T.text[k] = (char)ch; T.best[k] = (uint16_t)best; T.second[k] = (uint16_t)second; T.tmpl[k] = (uint8_t)tm; }
		}
		if (lane == 0u) {
			const uint32_t m = label_meters(T.text, ng);
			T.meters = m;
			S.meters[wave] = m;
		}
	}
	__syncthreads();

	// ---- 4. frame ----
	if (tid == 0u) {
		uint32_t bad = 0;
		double mpx = 0.0;
		S.rec.n = n;
		if (!label_anchors(F->label, n, S.meters, &S.rec.anchors, &mpx, &bad)) {   // (a label of k_scale_labels has a bar: not reached)
			S.rec.anchors.n = 0u; S.rec.anchors.scales_start_y = 0u;
			for (uint32_t k = 0; k < (uint32_t)SMHV_MAX_SCALES; ++k) S.rec.anchors.scales[k][0] = S.rec.anchors.scales[k][1] = S.rec.anchors.scales[k][2] = 0u;
			mpx = 0.0;
		}
		S.rec.has = S.rec.anchors.n ? 1u : 0u;
		S.rec.mpx = mpx;
	}
	__syncthreads();

	// ---- 5. output ----
	constexpr uint32_t REC_WORDS = sizeof(smhv_label_text_frame) / 4u, AN_WORDS = sizeof(smhv_anchors) / 4u;
	static_assert(REC_WORDS + AN_WORDS <= LT_THREADS, "a dword per thread");
	if (tid < REC_WORDS) ((uint32_t *)(r.out + f))[tid] = ((const uint32_t *)&S.rec)[tid];
	else if (tid < REC_WORDS + AN_WORDS) ((uint32_t *)(r.anchors + f))[tid - REC_WORDS] = ((const uint32_t *)&S.rec.anchors)[tid - REC_WORDS];
}

hipError_t launch_label_text(const LabelTextRun &r, uint32_t n, hipStream_t s) {
	if (n == 0u || !r.labels || !r.crops || !r.atlas || !r.out || !r.anchors) return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_label_text, dim3(n), dim3(LT_THREADS), 0, s, r);
	return hipGetLastError();
}

}  // namespace smh
