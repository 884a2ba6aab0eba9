// smh_record.inc -- the per-frame record: calc_meters_to_px_ratio (src/vision/mpx_ratio.rs:3-134) and the derived marker
// outputs (src/ui/mod.rs:131-140, markers.rs:98).  Device code shared by the record kernels of smh_misc.hip (k_scale_ratio,
// k_finalize, k_scales_finalize) and by k_lsd_tile, whose workgroups write their frame's record themselves when the batch
// asks for it (Buffers::rec_stages): one kernel less in every batch's chain on its hardware queue.
#pragma once
#include "smh_device.h"
#include "smh_firing.h"

namespace smh {

// ------------------------------------------------------------------------------------------------
// k_scale_ratio: src/vision/mpx_ratio.rs.  One wave per OCR label anchor (<= 3 per frame).  The scan
// order of the reference is kept (rows downwards from the anchor; first tick column to the right,
// then to the left), but each "first column whose 4 pixels below are all 0" search tests 64 columns
// per step and takes the first hit with a ballot.  Pixels below the image count as non-zero
// (reference: unchecked read).
// ------------------------------------------------------------------------------------------------
__device__ inline bool find_scale_width(const uint8_t *img, size_t pitch, uint32_t w, uint32_t h, uint32_t meters, uint32_t x, uint32_t y, double *ratio,
                                 uint32_t bar[3]) {
	const uint32_t lane = threadIdx.x & 63u;
	if (y < SMH_MIN_SCALE_VERTICAL_BAR_HEIGHT || x >= w) return false;
	// ((20.0 / 640.0) * w as f64).round(): 0.03125*w has at most 5 fractional bits, so t + 0.5 is exact
	// and floor(t + 0.5) is round-half-away-from-zero for t >= 0
	const double t = (20.0 / 640.0) * (double)w;
	const uint32_t max_off = (uint32_t)floor(t + 0.5);
	const uint32_t y_end = min(h, y + max_off);
	// "rows yy..yy+3 of column xx all 0" for 256 columns per step (four chunks of 64, sixteen independent loads per lane in flight
	// together, then the chunks' ballots in the search's order): a scale bar's tick sits 60-180 columns from its label, and a wave
	// of the search service pays every dependent round trip of this scan beside a saturated streaming pass (~2.5 us each).
	// col(i) = the i-th column of the search, i < count.  -> index of the first hit, or count
	auto first_tick = [&](uint32_t yy, uint32_t count, auto col) -> uint32_t {
		for (uint32_t base = 0; base < count; base += 256u) {
			uint8_t v[4][SMH_MIN_SCALE_VERTICAL_BAR_HEIGHT];
#pragma unroll
			for (uint32_t c = 0; c < 4u; ++c) {
				const uint32_t i = base + c * 64u + lane, xx = col(min(i, count - 1u));
#pragma unroll
				for (uint32_t k = 0; k < SMH_MIN_SCALE_VERTICAL_BAR_HEIGHT; ++k) v[c][k] = img[(size_t)min(yy + k, h - 1u) * pitch + xx];
			}
#pragma unroll
			for (uint32_t c = 0; c < 4u; ++c) {
				const uint32_t i = base + c * 64u + lane;
				uint32_t bad = 0;
#pragma unroll
				for (uint32_t k = 0; k < SMH_MIN_SCALE_VERTICAL_BAR_HEIGHT; ++k) bad |= (yy + k >= h || v[c][k] != 0) ? 1u : 0u;
				const uint64_t hit = __ballot(i < count && bad == 0u);
				if (hit) return base + c * 64u + (uint32_t)__builtin_ctzll(hit);
			}
		}
		return count;
	};
	// the rows below the anchor whose pixel in column x is 0, 64 rows per load (the reference tests them one after the other:
	// thirty dependent loads for a bar that sits at the end of the range), then in the reference's order
	for (uint32_t y0 = y; y0 < y_end; y0 += 64u) {
		const uint32_t yl = y0 + lane;
		uint64_t rows = __ballot(yl < y_end && img[(size_t)min(yl, h - 1u) * pitch + x] == 0);
		while (rows) {
			const uint32_t yy = y0 + (uint32_t)__builtin_ctzll(rows);
			rows &= rows - 1ull;
			const uint32_t ri = first_tick(yy, w - x, [&](uint32_t i) { return x + i; });                 // Go right...
			uint32_t right = ri < w - x ? x + ri : 0u;
			if (right == 0) continue;
			right -= 1;
			const uint32_t li = x ? first_tick(yy, x, [&](uint32_t i) { return x - 1u - i; }) : 0u;        // Go left... (columns x-1, x-2, ...)
			uint32_t left = li < x ? x - 1u - li : 0u;
			if (left == 0) continue;
			left += 1;
			const uint32_t width = right - left;   // wraps like release Rust (mpx_ratio.rs:58)
			if (width < SMH_MIN_SCALE_WIDTH) continue;
			bar[0] = left; bar[1] = yy; bar[2] = right;
			*ratio = (double)meters / (double)width;
			return true;
		}
	}
	return false;
}

// (a block of whole waves, any number of them: the waves take the label anchors in turn; ends with the result in
// results[f].has_mpx / mpx, written by thread 0)
__device__ __forceinline__ void scale_ratio_body(const Geom &g, const Buffers &b, uint32_t f, uint32_t *bars) {
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, nwaves = blockDim.x >> 6;
	__shared__ double s_ratio[SMHV_MAX_SCALES];
	__shared__ uint32_t s_ok[SMHV_MAX_SCALES];
	smhv_frame_result *res = &b.results[f];
	const bool open = b.aux[f].open != 0;
	const smhv_anchors an = b.anchors[f];
	const uint32_t n = open ? min(an.n, (uint32_t)SMHV_MAX_SCALES) : 0u;
	const bool valid = an.scales_start_y <= g.qh;
	for (uint32_t k = wave; k < SMHV_MAX_SCALES; k += nwaves) {   // wave-uniform
		double r = 0.0;
		uint32_t bar[3] = {0, 0, 0};
		bool ok = false;
		if (k < n && valid) {
			const uint8_t *img = b.scales + (size_t)f * g.ocr_stride + g.q_xoff;
			ok = find_scale_width(img, g.ocr_pitch, g.qw, g.qh, an.scales[k][0], an.scales[k][1], an.scales[k][2], &r, bar);
		}
		if (lane == 0) {
			s_ratio[k] = r; s_ok[k] = ok ? 1u : 0u;
			if (bars) {
				uint32_t *o = bars + ((size_t)f * SMHV_MAX_SCALES + k) * 4;
				o[0] = bar[0]; o[1] = bar[1]; o[2] = bar[2]; o[3] = ok ? 1u : 0u;
			}
		}
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		// the "Rayon ladder" (mpx_ratio.rs:93-125): mean of the successes, summed in index order
		double sum = 0.0; uint32_t k = 0;
		for (uint32_t i = 0; i < SMHV_MAX_SCALES; ++i)
			if (s_ok[i]) { sum = k ? sum + s_ratio[i] : s_ratio[i]; ++k; }
		res->has_mpx = k ? 1u : 0u;
		res->mpx = k == 0 ? 0.0 : (k == 1 ? sum : sum / (double)k);
	}
}

// ------------------------------------------------------------------------------------------------
// k_finalize: per-frame record header + ui::Marker::new / angle (src/ui/mod.rs:131-140, markers.rs:98)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void finalize_body(const Geom &g, const Buffers &b, uint32_t f, uint32_t stages, uint32_t l) {
	smhv_frame_result *res = &b.results[f];
	const FrameAux aux = b.aux[f];
	const bool open = aux.open != 0;
	const bool markers = (stages & SMHV_STAGE_MARKERS) != 0;
	const uint32_t n = (open && markers) ? res->n_lines : 0u;
	const bool has_mpx = open && (stages & SMHV_STAGE_SCALES) && res->has_mpx;
	const double mpx = has_mpx ? res->mpx : 0.0;
	if (l < SMHV_MAX_LINES) {
		double len = 0.0, met = 0.0;
		float ang = 0.0f;
		smhv_line ln = {0.0f, 0.0f, 0.0f, 0.0f};
		if (l < n) {
			ln = res->lines[l];
			const double ax = (double)ln.x0 - (double)ln.x1, ay = (double)ln.y0 - (double)ln.y1;
			len = sqrt(ax * ax + ay * ay);
			met = has_mpx ? len * mpx : 0.0;
			ang = atan2f(ln.y0 - ln.y1, ln.x0 - ln.x1);
		}
		res->lines[l] = ln;
#ifdef SMH_LSD_PROFILE
		if (l < 20)
#endif
		res->length_px[l] = len;
#ifdef SMH_LSD_PROFILE
		if (l < 16)
#endif
		res->angle[l] = ang;
#ifdef SMH_LSD_PROFILE
		if (l < 20)
#endif
		res->meters[l] = met;
	}
	if (l == 0) {
		res->map_open = open ? 1u : 0u;
		res->n_lines = n;
		res->mpx = mpx; res->has_mpx = has_mpx ? 1u : 0u;
		res->n_mask_px = (open && markers) ? aux.n_mask_px : 0u;
		res->red_pixels = aux.red;
		if (!(open && markers)) { res->rounds = 0; res->ray_steps = 0; }
		if (!(stages & SMHV_STAGE_MINIMAP)) { res->has_minimap = 0; res->minimap[0] = 0; res->minimap[1] = 0; res->minimap[2] = 0; res->minimap[3] = 0; }
		if (!(open && markers)) res->status = SMHV_FRAME_OK;          // otherwise the line search's verdict stands
	}
}

__device__ __forceinline__ void finalize_body(const Geom &g, const Buffers &b, uint32_t f, uint32_t stages) { finalize_body(g, b, f, stages, threadIdx.x); }

// SMHV_STAGE_FIRING after finalize_body, by the wave that wrote the record: lane 0's header has left before the lanes read it back
__device__ __forceinline__ void firing_after_finalize(const Buffers *bp, uint32_t f, uint32_t lane) {
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
	firing_frame_tail(bp, f, lane);
}

// scale ratio + record by ONE workgroup of at least 64 threads, any size (the waves take the label anchors in turn); every
// thread of the workgroup must call it, after a barrier behind the line search's own writes of the record
__device__ __attribute__((noinline)) void frame_record_tail(const Geom *gp, const Buffers *bp, uint32_t f) {
	const Geom &g = *gp;
	const Buffers &b = *bp;
	const uint32_t stages = b.rec_stages & ~SMH_REC_ON;
	if (stages & SMHV_STAGE_SCALES) {
		scale_ratio_body(g, b, f, b.rec_bars);
		__syncthreads();                                       // thread 0's has_mpx / mpx are visible to the block
	}
	if (threadIdx.x < 64) {
		finalize_body(g, b, f, stages);
		if (stages & SMHV_STAGE_FIRING) firing_after_finalize(bp, f, threadIdx.x);
	}
}

// The same by ONE WAVE of a workgroup whose other waves are busy with other frames (k_lsd_service): the wave takes the label
// anchors one after the other (every lane holds the same ratios: find_scale_width's verdicts are ballots), then the record.
__device__ __attribute__((noinline)) void frame_record_tail_wave(const Geom *gp, const Buffers *bp, uint32_t f) {
	const Geom &g = *gp;
	const Buffers &b = *bp;
	const uint32_t stages = b.rec_stages & ~SMH_REC_ON;
	const uint32_t lane = threadIdx.x & 63u;
	smhv_frame_result *res = &b.results[f];
	if (stages & SMHV_STAGE_SCALES) {
		const bool open = b.aux[f].open != 0;
		const smhv_anchors an = b.anchors[f];
		const uint32_t n = open ? min(an.n, (uint32_t)SMHV_MAX_SCALES) : 0u;
		const bool valid = an.scales_start_y <= g.qh;
		double sum = 0.0;
		uint32_t cnt = 0;
		for (uint32_t k = 0; k < SMHV_MAX_SCALES; ++k) {
			double r = 0.0;
			uint32_t bar[3] = {0, 0, 0};
			bool ok = false;
			if (k < n && valid) {
				const uint8_t *img = b.scales + (size_t)f * g.ocr_stride + g.q_xoff;
				ok = find_scale_width(img, g.ocr_pitch, g.qw, g.qh, an.scales[k][0], an.scales[k][1], an.scales[k][2], &r, bar);
			}
			if (lane == 0 && b.rec_bars) {
				uint32_t *o = b.rec_bars + ((size_t)f * SMHV_MAX_SCALES + k) * 4;
				o[0] = bar[0]; o[1] = bar[1]; o[2] = bar[2]; o[3] = ok ? 1u : 0u;
			}
			if (ok) { sum = cnt ? sum + r : r; ++cnt; }        // the "Rayon ladder" (mpx_ratio.rs:93-125): summed in index order
		}
		if (lane == 0) {
			res->has_mpx = cnt ? 1u : 0u;
			res->mpx = cnt == 0 ? 0.0 : (cnt == 1 ? sum : sum / (double)cnt);
		}
	}
	// lane 0's n_lines / has_mpx / mpx have left before the other lanes read them back
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
	finalize_body(g, b, f, stages, lane);
	if (stages & SMHV_STAGE_FIRING) firing_after_finalize(bp, f, lane);   // (before the service counts the frame off)
}

}  // namespace smh
