// smh_yuvout.hip -- RGBA8 / BGRA8 images (and the grey ui_map's luma plane) -> 8-bit 4:2:0 video frames (NV12 / I420), the
// layouts a hardware encoder takes (include/smh_vision_hip.h, "video frames OUT"; the arithmetic is pinned there).
//
// Streaming: 4 bytes in (1 from the luma plane), 1.5 bytes out per pixel.  A lane converts a block of 2 rows x 8 pixels whose x is
// a multiple of 8 and whose y is even, so the block owns one chroma row and four chroma columns: four 16-byte loads (two dwords
// per row from the luma plane), 8 Y bytes per row, and 8 bytes of U, V pairs (NV12) or 4 bytes into each chroma plane (I420).
// Sources are pitched with any 4-byte alignment, which the 16-byte loads take as it is; destinations have any byte alignment, so
// every store has two forms: dwords where the address allows it and the block lies wholly inside the image, bytes otherwise.  A
// block at the right edge loads single pixels, and the luma plane is read in the aligned dwords its bytes lie in.  At an odd
// right or bottom edge the pixel loads are clamped, which is the header's "an edge pixel counts twice".  Grid-stride over
// (frame, row pair, column group), the column group fastest: a wave reads 2 KB of a row and the 2 KB below it.
// No LDS, no scratch: every array below is indexed by unrolled constants.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "smh_kernels.h"

namespace smh {

// four pixels at any 4-byte alignment: one global_load_dwordx4 (global memory takes 16-byte accesses at dword alignment)
typedef uint32_t yo_u32x4 __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ uint32_t yo_clip8(int v) { return (uint32_t)min(max(v, 0), 255); }
__device__ __forceinline__ uint32_t yo_pack4(const uint32_t *v) { return v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24); }

// the 8 bytes at p (any alignment), of which the first nv (1 .. 8) are wanted: the aligned dwords that hold a wanted byte, shifted
// into place (the others are not read; what the result holds beyond byte nv - 1 is not used)
__device__ __forceinline__ uint2 yo_load8(const uint8_t *p, uint32_t nv) {
	const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
	const uint32_t *q = (const uint32_t *)(p - sh);
	const uint32_t d0 = q[0], d1 = sh + nv > 4u ? q[1] : 0u, d2 = sh + nv > 8u ? q[2] : 0u;
	return make_uint2(__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh));
}

template <int LAYOUT>
__global__ void __launch_bounds__(256) k_bgra_to_yuv420(const YuvOutRun run) {
	const YuvOutCoef k = run.k;
	const uint32_t rs = run.rgba ? 0u : 16u, bs = 16u - rs;   // where R and B lie in a pixel's dword
	const int T = k.yr + k.yg + k.yb;
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < run.items; i += gridDim.x * 256u) {
		const uint32_t t = i / run.groups, g = i - t * run.groups;
		const uint32_t f = t / run.pairs, pr = t - f * run.pairs;
		const uint32_t x = g << 3, y = pr << 1;
		const uint32_t nv = min(8u, run.w - x);                // valid columns of the block
		const bool full = nv == 8u, row1 = y + 1u < run.h;
		const bool from_luma = run.form ? run.form[f] == UI_FORM_LUMA : run.src == nullptr;
		uint32_t Y[2][8], U[4], V[4];
		if (from_luma) {
			// grey: Y from the one byte, chroma the constant 128 (the header's "grey pixels")
			const uint8_t *p = run.luma + (size_t)f * run.luma_stride + (size_t)y * run.luma_pitch + x;
#pragma unroll
			for (int r = 0; r < 2; ++r) {
				uint2 v = make_uint2(0u, 0u);
				if (r == 0 || row1) v = yo_load8(p + (size_t)r * run.luma_pitch, nv);
#pragma unroll
				for (int j = 0; j < 8; ++j) {
					const int l = (int)(((j < 4 ? v.x : v.y) >> (8 * (j & 3))) & 255u);
					Y[r][j] = yo_clip8(((T * l + 32768) >> 16) + k.yoff);
				}
			}
#pragma unroll
			for (int c = 0; c < 4; ++c) U[c] = V[c] = 128u;
		} else {
			const uint8_t *p = run.src + (size_t)f * run.src_stride + (size_t)y * run.src_pitch;
			// rows y and y + 1; at the bottom edge of an odd height row y again, at the right edge of an odd width column w - 1 again
			const uint32_t *row0 = (const uint32_t *)p, *row1p = (const uint32_t *)(p + (row1 ? run.src_pitch : 0u));
			uint32_t px[2][8];
			if (full) {
				// All four loads in flight at once.  Non-temporal: the pixels are read once -- and hipcc merges plain loads here with the
				// single-pixel loads of the other arm into sixteen dword loads for both, which this keeps apart.
				const yo_u32x4 a0 = __builtin_nontemporal_load((const yo_u32x4 *)(row0 + x)), b0 = __builtin_nontemporal_load((const yo_u32x4 *)(row0 + x + 4u));
				const yo_u32x4 a1 = __builtin_nontemporal_load((const yo_u32x4 *)(row1p + x)), b1 = __builtin_nontemporal_load((const yo_u32x4 *)(row1p + x + 4u));
				px[0][0] = a0.x; px[0][1] = a0.y; px[0][2] = a0.z; px[0][3] = a0.w; px[0][4] = b0.x; px[0][5] = b0.y; px[0][6] = b0.z; px[0][7] = b0.w;
				px[1][0] = a1.x; px[1][1] = a1.y; px[1][2] = a1.z; px[1][3] = a1.w; px[1][4] = b1.x; px[1][5] = b1.y; px[1][6] = b1.z; px[1][7] = b1.w;
			} else {
#pragma unroll
				for (int j = 0; j < 8; ++j) {
					const uint32_t xc = min(x + (uint32_t)j, run.w - 1u);
					px[0][j] = row0[xc]; px[1][j] = row1p[xc];
				}
			}
			int R[2][8], G[2][8], B[2][8];
#pragma unroll
			for (int r = 0; r < 2; ++r)
#pragma unroll
				for (int j = 0; j < 8; ++j) {
					R[r][j] = (int)((px[r][j] >> rs) & 255u); G[r][j] = (int)((px[r][j] >> 8) & 255u); B[r][j] = (int)((px[r][j] >> bs) & 255u);
					Y[r][j] = yo_clip8(((k.yr * R[r][j] + k.yg * G[r][j] + k.yb * B[r][j] + 32768) >> 16) + k.yoff);
				}
#pragma unroll
			for (int c = 0; c < 4; ++c) {
				const int Rs = R[0][2 * c] + R[0][2 * c + 1] + R[1][2 * c] + R[1][2 * c + 1];
				const int Gs = G[0][2 * c] + G[0][2 * c + 1] + G[1][2 * c] + G[1][2 * c + 1];
				const int Bs = B[0][2 * c] + B[0][2 * c + 1] + B[1][2 * c] + B[1][2 * c + 1];
				U[c] = yo_clip8(((k.ur * Rs + k.ug * Gs + k.ub * Bs + 131072) >> 18) + 128);
				V[c] = yo_clip8(((k.vr * Rs + k.vg * Gs + k.vb * Bs + 131072) >> 18) + 128);
			}
		}
		uint8_t *dst = run.dst + (size_t)f * run.dst_stride;
#pragma unroll
		for (int r = 0; r < 2; ++r) {
			if (r == 1 && !row1) continue;
			uint8_t *o = dst + (size_t)(y + r) * run.y_pitch + x;
			if (full && ((uintptr_t)o & 3u) == 0u) { ((uint32_t *)o)[0] = yo_pack4(&Y[r][0]); ((uint32_t *)o)[1] = yo_pack4(&Y[r][4]); }
			else {
#pragma unroll
				for (int j = 0; j < 8; ++j) if ((uint32_t)j < nv) o[j] = (uint8_t)Y[r][j];
			}
		}
		const uint32_t cx = x >> 1, nc = (nv + 1u) >> 1;          // the block's first chroma column, its valid chroma columns
		if (LAYOUT == SMH_YUV_NV12) {
			uint8_t *o = dst + run.u_off + (size_t)pr * run.uv_pitch + 2u * (size_t)cx;
			if (full && ((uintptr_t)o & 3u) == 0u) {
				((uint32_t *)o)[0] = U[0] | (V[0] << 8) | (U[1] << 16) | (V[1] << 24);
				((uint32_t *)o)[1] = U[2] | (V[2] << 8) | (U[3] << 16) | (V[3] << 24);
			} else {
#pragma unroll
				for (int c = 0; c < 4; ++c) if ((uint32_t)c < nc) { o[2 * c] = (uint8_t)U[c]; o[2 * c + 1] = (uint8_t)V[c]; }
			}
		} else {
			uint8_t *ou = dst + run.u_off + (size_t)pr * run.uv_pitch + cx, *ov = dst + run.v_off + (size_t)pr * run.uv_pitch + cx;
			if (full && ((uintptr_t)ou & 3u) == 0u) *(uint32_t *)ou = yo_pack4(U);
			else {
#pragma unroll
				for (int c = 0; c < 4; ++c) if ((uint32_t)c < nc) ou[c] = (uint8_t)U[c];
			}
			if (full && ((uintptr_t)ov & 3u) == 0u) *(uint32_t *)ov = yo_pack4(V);
			else {
#pragma unroll
				for (int c = 0; c < 4; ++c) if ((uint32_t)c < nc) ov[c] = (uint8_t)V[c];
			}
		}
	}
}

// run: everything but the item counts, which are filled in here
hipError_t launch_bgra_to_yuv(YuvOutRun run, uint32_t layout, hipStream_t s) {
	run.groups = (run.w + 7u) / 8u; run.pairs = (run.h + 1u) / 2u;
	const uint64_t items = (uint64_t)run.groups * run.pairs * run.n;
	if (items == 0 || items > 0x7FFFFFFFull || (!run.src && !run.luma) || (run.form && (!run.src || !run.luma)) || (layout != SMH_YUV_NV12 && layout != SMH_YUV_I420))
		return hipErrorInvalidValue;
	run.items = (uint32_t)items;
	// memory-bound: at most 8 workgroups per CU's worth of blocks, the rest by the stride
	const dim3 grid((uint32_t)std::min<uint64_t>((items + 255u) / 256u, 2048u)), block(256);
	if (layout == SMH_YUV_NV12) hipLaunchKernelGGL((k_bgra_to_yuv420<SMH_YUV_NV12>), grid, block, 0, s, run);
	else hipLaunchKernelGGL((k_bgra_to_yuv420<SMH_YUV_I420>), grid, block, 0, s, run);
	return hipGetLastError();
}

}  // namespace smh
