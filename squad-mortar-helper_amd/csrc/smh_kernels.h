// smh_kernels.h -- launch interface between the host runtime (smh_runtime.cpp) and the gfx950
// kernels (smh_stream.hip, smh_lsd.hip, smh_misc.hip).  Internal; the public boundary is include/smh_vision_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/smh_vision_hip.h"
#include "../../include/smh_vision_hip_debug.h"

namespace smh {

// Geometry + device buffer layout of one frame size.  All buffers are per-batch slabs indexed by
// frame; rows are padded so that the 16-byte-per-lane accesses of the streaming passes are
// aligned: a "quad" is 4 horizontally adjacent pixels whose frame x is a multiple of 4, and the
// padded output rows start at the ROI's quad-aligned x (ROI pixel 0 sits `xoff` pixels in).
struct Geom {
	uint32_t W, H;                 // frame
	uint32_t rx, ry, rw, rh;       // map ROI (reference "cropped_map")
	uint32_t bx, by, bw, bh;       // close-deployment button
	uint32_t qx, qy, qw, qh;       // bottom-right quadrant in FRAME coordinates / size
	// map pass
	uint32_t m_ax, m_xoff, m_quads, m_block;   // aligned x, rx - ax, quads per row, threads per block
	// brq pass
	uint32_t q_ax, q_xoff, q_quads, q_block;
	// layouts (bytes unless noted)
	uint64_t frame_bytes;
	uint64_t ui_pitch, ui_stride;
	uint64_t mask_pitch, mask_stride;
	uint32_t bits_pitch_w; uint64_t bits_stride_w;  // words
	uint64_t ocr_pitch, ocr_stride;                // also used for the scales image
};

// per-frame scratch written by k_button / k_map_pass, read by k_lsd
struct FrameAux {
	uint32_t open;        // button test passed
	uint32_t red;         // red pixel count
	uint32_t n_mask_px;   // popcount of the dilated mask
	uint32_t y_min, y_max, w_min, w_max;  // bounding box of set bits: rows, and words of the bit-packed rows
	uint32_t tiles;       // 1: the pass that wrote this frame's mask also wrote it tile-major with occupancy bytes (bands of whole tile rows)
};

// ---- cooperation between the workgroups of one k_lsd launch (smh_lsd.hip) ---------------------------------------
// A frame's line scan is sequential, but casting the rays of a candidate pixel is a pure function of (mask, pixel):
// workgroups that have finished their own frame ("helpers") load the mask of a frame that is still being searched and
// ray-cast candidates its owner has posted ahead of its own position; the results travel back through a per-frame
// hash table keyed by the pixel.  The owner never waits for a helper and a missing result only means it casts itself,
// so the outputs are the sequential algorithm's bit for bit.
struct LsdCoop {             // one 64-byte line per frame, zeroed before every launch
	uint32_t req_tail;       // requests posted by the owner
	uint32_t req_head;       // requests claimed by helpers (the owner raises it to req_tail to cancel what is pending)
	uint32_t done;           // the owner has finished the frame
	uint32_t helpers;        // helpers attached
	uint32_t remaining;      // surviving candidate pixels the owner still has in front of it (what helpers go by)
	uint32_t mode1;          // 1 + mask residency mode of the owner's kernel (helpers of another mode's kernel keep off)
	uint32_t stat_groups, stat_hits, stat_casts;   // diagnostics: helped groups of the owner, cache hits, candidates cast by helpers
	uint32_t pad[7];
};
struct LsdCtl {              // per launch, zeroed with the LsdCoop array; [residency mode]
	uint32_t started[3];     // owner workgroups dispatched
	uint32_t finished[3];    // owner workgroups that have left their frame
	uint32_t pad[10];
};
struct LsdCacheEntry {       // 32 bytes
	unsigned long long tag;  // epoch << 32 | busy << 31 | y << 12 | x ; epoch identifies the launch (stale entries = empty)
	unsigned long long best; // max over rays of (len^2 bits << 32 | ray index)
	float ex, ey;            // end point of that ray
	uint32_t steps, pad;     // mask samples of all rays of the candidate
};
#define SMH_LSD_REQ_CAP 64u          // request ring entries per frame (seq << 24 | y << 12 | x)
#define SMH_LSD_CACHE_SLOTS 512u     // hash slots per frame
struct LsdCoopBufs {
	LsdCtl *ctl;             // null: no cooperation (Vision::find_longest_line, or the buffers are absent)
	LsdCoop *coop;
	uint32_t *req;           // n x SMH_LSD_REQ_CAP
	LsdCacheEntry *cache;    // n x SMH_LSD_CACHE_SLOTS
	uint32_t epoch;
};

// Error mailbox of a batch: pinned host memory mapped into the device, written by the device only when a frame fails
// (SMHV_FRAME_*), read by the host after it has synchronised with the run (smhv_batch_read_results, smhv_pipeline_wait,
// smhv_node_gather).  Sticky until reported.
struct BatchError {
	uint32_t count;          // frames whose status is not SMHV_FRAME_OK since the last report
	uint32_t frame, status;  // the first of them
	uint32_t info[8];        // SMHV_FRAME_LSD_STUCK: head, tail, disp_e, disp_end, n_lines, rounds, spec, state of the head slot
	uint32_t pad[5];
};

// ---- late helpers of k_lsd_tile (round 3) ---------------------------------------------------------------------------------
// A workgroup that has written its own frame's record looks once over the launch's frames, takes one that is still at work and
// has asked for help (FarmFrame::want), builds the same tile store and casts whole CANDIDATES its owner posts to it: the owner's
// reorder buffer holds local and remote candidates alike and retires them in order, so lines, rounds and sample counts are the
// sequential scan's whichever workgroup cast a candidate (casting is a pure function of (mask, pixel)).  Every word below is ONE
// 8-byte agent-scope atomic (a granule is never torn, needs no fence); the three payload words of a result are stored, drained
// (s_waitcnt vmcnt(0)), then the tagged word.
#define SMH_FARM_RING 4u
#define SMH_REC_ON 0x80000000u
#define SMH_LSD_LATE_HELP 1u
struct FarmEntry {                  // 64 bytes
	unsigned long long post;        // owner -> helper: epoch16 << 48 | (k + 1)24 << 24 | py12 << 12 | px12   (k = posts so far)
	unsigned long long best;        // helper -> owner: max over rays of (len^2 bits << 32 | ray index)
	unsigned long long end;         //   ey bits << 32 | ex bits
	unsigned long long start;       //   pty bits << 32 | ptx bits
	unsigned long long done;        //   tag32 << 32 | steps, tag = epoch16 << 16 | (k + 1)16: written last
	unsigned long long pad[3];
};
struct FarmFrame {                  // one per frame of the launch
	unsigned long long attached;    // helper -> owner: epoch when the helper has built its tile store and listens
	unsigned long long owner_done;  // owner -> helper: epoch when the frame is finished
	// late helpers (SMH_LSD_LATE_HELP): a workgroup that has finished its own frame helps one that is still at work
	unsigned long long want;        // owner -> anybody: epoch16 << 48 | survivor-list entries still to visit (refreshed now and then)
	unsigned long long claimed;     // finished workgroup -> the others: epoch when one of them has taken this frame (compare-and-swap)
	unsigned long long pad[4];
	FarmEntry ring[SMH_FARM_RING];
};

struct Buffers {
	BatchError *err;         // device address of the batch's mailbox (null: none)
	FarmFrame *farm;         // late-helper exchange of k_lsd_tile, one entry per frame (null: none)
	// k_lsd_tile writes the frame's record itself (smh_record.inc: scale ratio + derived marker outputs) when SMH_REC_ON is set:
	// rec_stages = SMH_REC_ON | the run's stage mask (SMHV_STAGE_SCALES cleared when the run has no anchors), rec_bars = the
	// scale-bar debug slab or null
	uint32_t rec_stages;
	uint32_t *rec_bars;
	uint32_t lsd_flags, lsd_late_kc; // SMH_LSD_LATE_HELP: `farm` holds one entry per frame and finished workgroups help frames still at work
	                                 // lsd_late_kc x 1024 cycles after they began
	const uint8_t *frames;   // n * frame_bytes
	uint8_t *ui, *mask, *ocr, *scales;
	uint32_t *bits;
	// the same mask tile-major, and which tiles hold a set bit (written by the streaming passes, read by the search service's
	// tile-store builder: tiled_* / occ_* below)
	uint32_t *tiled;
	uint8_t *occ;
	FrameAux *aux;
	smhv_frame_result *results;
	const smhv_anchors *anchors;   // device copy, may be null
	// k_lsd sector culling table for this max_gap (null: cast every ray), SMH_CULL_TAB_WORDS words:
	//   [SMH_CULL_CELLS words] cell (row oy + R) * 4 + j: mask of the OUTER annulus' pixels among offsets ox = -R + 32 j + [0, 32)
	//   [SMH_CULL_CELLS words] -DSMH_CULL_CHAIN only: the same of the MIDDLE annulus (all zero where the threshold has none: the cull is then not chained)
	//   [(2R+1)^2 bytes, row-major] unit range of each annulus pixel: first_unit | (n_units - 1) << 6, 0xFF = every unit
	const uint32_t *cull_tab;
	// x/y offsets of every ray after 32 j additions of its direction, j = 0..SMH_RAY_OFF_BATCHES (float2 [3600][SMH_RAY_OFF_BATCHES + 1];
	// built on the device with the reference's own repeated f32 addition): lets several lanes walk different 32-sample
	// batches of ONE long ray at the same time (k_lsd_wave).  null: long rays are walked batch after batch.
	const float *ray_off;
	LsdCoopBufs co;
	// SMHV_STAGE_FIRING: the run's firing parameters (smh_firing.h), a per-batch block uploaded with the run (null: no firing)
	const struct FiringRun *firing;
};
// Per-run parameters of the firing solutions (smh_firing.h): what smhv_batch_set_firing / smhv_pipeline_set_firing bound when the
// run was enqueued, and the batch's firing slab.  Uploaded from pinned staging with the run, so a submission in flight keeps its own.
struct FiringRun {
	const uint16_t *hm;            // heightmap texels, row-major (null: none bound)
	smhv_firing_result *out;       // the batch's firing slab, one entry per frame
	uint32_t hm_w, hm_h;
	float b0x, b0y;                // bounds[0] as f32
	double zscale;                 // scale[2] as f64 / 0.1953125
	uint32_t flags;                // SMHV_FIRING_*
	float sw, sh, tx, ty;          // map viewport: scale factors and top left
	uint32_t pad;
};
static_assert(sizeof(FiringRun) == 64, "one 64-byte block per run");
// SMHV_STAGE_HEIGHTMAP_OVERLAY / smhv_heightmap_overlay (k_hm_overlay): the heightmap's colours drawn over the ui_map of n frames.
// Launch arguments (taken by value at the launch: a submission in flight keeps its own); the slabs have the ui slab's layout.
struct OverlayRun {
	const uint8_t *ui;                   // the ui slab, frame 0
	uint8_t *out;                        // the overlay slab, frame 0
	const FrameAux *aux;                 // per frame: open (the record's map_open is written after the overlay has run)
	const smhv_frame_result *res;        // per frame: has_minimap, minimap (written by k_find_minimap before the overlay)
	const uint16_t *hm;                  // heightmap texels, row-major
	const uint32_t *lut;                 // 65,536 RGBA8 colours: lut[v] = the colour map's colour of a texel v (smh_misc.hip, k_hm_lut)
	uint32_t hm_w, hm_h;
	float b0x, b0y;                      // bounds[0] as f32
	uint32_t flags;                      // SMHV_FIRING_BOUNDS_OFFSET
};
// smhv_batch_render / smhv_render_map (k_render_map, smh_render.hip): the app's map view of n frames at one viewport.  Launch
// arguments, taken by value at the launch.
#define SMH_RND_MAX_LINES 256u           // explicit lines of smhv_render_map (a record holds at most SMHV_MAX_LINES)
struct RenderRun {
	const uint8_t *ui;                   // the ui slab, at the first frame of the call
	uint8_t *out;                        // the render slab, at the first frame of the call: out_w x out_h RGBA8, tightly packed
	const FrameAux *aux;                 // per frame: open
	const smhv_frame_result *res;        // per frame: has_minimap, minimap, n_lines, lines
	const smhv_line *lines;              // explicit lines for every frame of the call (null: the record's)
	const uint16_t *hm;                  // heightmap texels, row-major (null: none)
	const uint32_t *lut;                 // its colour table (hm_lut); word SMH_HM_LUT_ENTRIES + 2 = vr of the 16-bit table
	const uint16_t *lut16;               // the same colours in 16 bits (k_hm_lut16), what the table form keeps in LDS
	uint64_t out_stride;                 // out_w * out_h * 4
	uint32_t hm_w, hm_h;
	float b0x, b0y;                      // bounds[0] as f32
	uint32_t flags;                      // SMHV_RENDER_*
	uint32_t n_lines;                    // of `lines`
	uint32_t out_w, out_h;
	float ql, qt, qr, qb;                // the map quad
	float sw, sh, tx, ty;                // the viewport: scale factors and top left
	uint32_t bg;                         // background, RGBA8 as a little-endian word
	uint32_t lds_texels;                 // set by the launcher: texels of LDS of the staged form (0: another form)
	uint32_t n_frames;                   // set by the launcher
};
// The layers of smhv_batch_render_layers / smhv_render_map_layers (k_render_map_layers): a further launch argument, so RenderRun
// and the kernels that take it alone stay what they were.
#define SMH_RND_MAX_ITEMS (SMH_RND_MAX_LINES + SMHV_RENDER_MAX_PRIMS + 1u)   // the kernel's LDS list: lines, prims, the minimap bounds
#define SMH_RND_SRC_UI 0u                // step 1 samples the ui slab (RenderRun::ui)
#define SMH_RND_SRC_GRAY 1u              //   ... a plane of one byte per pixel at `src` (the ocr, scales or mask slab): (L, L, L, 255)
#define SMH_RND_SRC_RGBA 2u              //   ... one RGBA8 image at `src` for the call's single frame (the per-call path's debug view)
#define SMH_RND_SRC_PREPROCESS 3u        //   ... the colour ui slab, every pixel that is no marker black
#define SMH_RND_SRC_CROPPED 4u           //   ... the colour ui slab's bottom right quarter
struct RenderLayersRun {
	const smhv_render_prim *prims;       // device memory: the prims without SMHV_PRIM_FOREGROUND in list order, then those with it
	const uint8_t *src;                  // SRC_GRAY: the slab at the first frame of the call; SRC_RGBA: the image
	uint64_t src_pitch, src_stride;      // bytes per row and per frame of `src`
	uint32_t src_xoff;                   // SRC_GRAY: bytes from a row's start to its first pixel
	uint32_t src_mode;                   // SMH_RND_SRC_*
	uint32_t src_w, src_h;               // the size of step 1's texture, whichever it is
	uint32_t n_below, n_fg;              // prims of either kind
	uint32_t flags;                      // SMHV_LAYER_*
	uint32_t pad;
};
// smhv_batch_render_labels / smhv_render_map_labeled (k_label_plan, k_label_draw: smh_labels.hip): the marker labels of n frames.
// Launch arguments, taken by value at the launch.
#define SMH_LBL_SLOTS (SMHV_LABEL_MAX_EXTRA + SMHV_MAX_LINES)
struct LabelCull { float mx, my, rad; uint32_t live; };   // per slot, for k_label_draw's cull: the midpoint, the circle that holds every painted pixel, n_runs != 0
struct LabelRun {
	FiringRun fr;                        // the heightmap and the viewport, as the firing solutions take them (`out` is not used)
	const FrameAux *aux;                 // per frame: open
	const smhv_frame_result *res;        // per frame: the minimap rectangle; batch: m/px, meters and the detected lines too
	const smhv_label_line *extra;        // device memory: the call's extra lines
	const smhv_line *lines;              // per call: the explicit detected lines (null: the record's)
	smhv_label_result *out;              // the label slab, at the first frame of the call
	LabelCull *cull;                     // SMH_LBL_SLOTS entries per frame, at the first frame of the call
	uint8_t *img;                        // the render slab, at the first frame of the call
	uint64_t img_stride;                 // out_w * out_h * 4
	double mpx;                          // per call: the frame's meters per pixel (valid iff has_mpx)
	uint32_t out_w, out_h;
	uint32_t n_extra, n_lines;           // of `extra`, of `lines`
	uint32_t detected;                   // SMHV_LABEL_DETECTED
	uint32_t scale;                      // S, 1 .. 4
	uint32_t per_call;                   // 1: `lines`, `mpx` / has_mpx are the call's and res is one record for the rectangle alone
	uint32_t has_mpx;
};
// smhv_batch_reach / smhv_reach_map (k_reach: smh_reach.hip): the reach map of n frames.  Launch arguments, taken by value at the
// launch.  T_j = tan(mils_j * pi / 3200), mils_j = 900 .. 1500, from glibc's tan (the header's "reach map"; never computed at run time).
#define SMH_REACH_THRESHOLDS {0x1.37efd8d87607ep+0, 0x1.7f218e25a745fp+0, 0x1.def13b73c1408p+0, 0x1.3504f333f9de6p+1, 0x1.a5f59e90600d8p+1, \
                              0x1.41bfee2424769p+2, 0x1.44e6c595afdc2p+3}
#define SMH_REACH_TW 64u                 // a workgroup's tile: one column per lane ...
#define SMH_REACH_ROWS 4u                //   ... and this many rows per wave, four waves
#define SMH_REACH_TH (4u * SMH_REACH_ROWS)
struct ReachRun {
	FiringRun fr;                        // the heightmap and the viewport, as the firing solutions take them (`out` is not used)
	const FrameAux *aux;                 // batch, per frame: open
	const smhv_frame_result *res;        // batch, per frame: m/px, the minimap rectangle, the lines (the origin)
	smhv_reach_result *out;              // the reach slab, at the first frame of the call; cleared ahead of the launch
	uint8_t *img;                        // PAINT: the render slab, at the first frame of the call
	uint8_t *cls;                        // CLASSES: out_w * out_h bytes per frame
	uint64_t img_stride, cls_stride;     // out_w * out_h * 4, out_w * out_h
	double mpx;                          // per call: the frame's meters per pixel (valid iff has_mpx)
	double ring_m;
	float origin[2];                     // SMHV_REACH_ORIGIN_POINT
	uint32_t mm[4];                      // per call: the minimap rectangle (valid iff has_mm)
	uint32_t out_w, out_h;
	uint32_t origin_mode, line;
	uint32_t per_call, has_mpx, has_mm;  // 1: mpx / has_mpx, mm / has_mm are the call's and aux, res are not read
	uint32_t pal[10];                    // out_of_range, band[0 .. 7], ring: R, G, B, a as a little-endian word
};
// smhv_batch_clearance / smhv_clearance_lines (k_clear_lines: smh_clear.hip): the terrain clearance of the lines of n frames, or of
// explicit lines.  Launch arguments, taken by value at the launch.
#define SMH_CLEAR_PROFILE (SMHV_CLEAR_MAX_SAMPLES + 1u)   // floats of a line's profile row
struct ClearLinesRun {
	FiringRun fr;                        // the heightmap and the viewport, as the firing solutions take them (`out` is not used)
	const smhv_frame_result *res;        // batch, per frame: n_lines, the lines, the minimap rectangle (as firing_frame_tail reads them)
	const smhv_line *lines;              // per call: the explicit lines
	smhv_clearance_result *out;          // batch: the clearance slab, at the first frame of the call
	smhv_clearance *out_lines;           // per call: one record per line
	float *profiles;                     // SMH_CLEAR_PROFILE floats per line, SMHV_MAX_LINES lines per frame (per call: per line); null: none
	double margin_m;
	uint32_t samples;                    // S
	uint32_t n_lines;                    // per call: of `lines`
	uint32_t mm[4];                      // per call: the minimap rectangle (valid iff has_mm)
	uint32_t per_call, has_mm;
};
// smhv_batch_clearance_map / smhv_clearance_map (k_clear_map: smh_clear.hip): the clearance map of n frames, in k_reach's tiles.
#define SMH_CLEAR_KC 32u                 // samples whose texel coordinates a workgroup stages in LDS at a time
struct ClearMapRun {
	FiringRun fr;
	const FrameAux *aux;                 // batch, per frame: open
	const smhv_frame_result *res;        // batch, per frame: the minimap rectangle, the lines (the origin)
	smhv_clearance_map_result *out;      // the clearance-map slab, at the first frame of the call; cleared ahead of the launch
	uint8_t *img;                        // PAINT: the render slab, at the first frame of the call
	uint8_t *bytes;                      // BYTES: out_w * out_h bytes per frame
	uint64_t img_stride, bytes_stride;   // out_w * out_h * 4, out_w * out_h
	double margin_m;
	float origin[2];                     // SMHV_REACH_ORIGIN_POINT
	uint32_t mm[4];                      // per call: the minimap rectangle (valid iff has_mm)
	uint32_t out_w, out_h;
	uint32_t samples;                    // S
	uint32_t origin_mode, line;
	uint32_t per_call, has_mm;           // 1: mm / has_mm are the call's and aux, res are not read
	uint32_t pal[4];                     // out_of_range, clear, blocked, los: R, G, B, a as a little-endian word
};
// smhv_batch_relief / smhv_relief_map (k_relief, k_relief_finish: smh_relief.hip): the terrain relief of n frames, in k_reach's tiles.
struct ReliefRun {
	FiringRun fr;                        // the heightmap and the viewport, as the firing solutions take them (`out` is not used)
	const FrameAux *aux;                 // batch, per frame: open
	const smhv_frame_result *res;        // batch, per frame: the minimap rectangle
	smhv_relief_result *out;             // the relief slab, at the first frame of the call; cleared ahead of the launch
	uint8_t *img;                        // PAINT: the render slab, at the first frame of the call
	uint8_t *bytes, *shades;             // the planes (null: not asked for): out_w * out_h elements per frame
	float *heights;
	uint64_t img_stride, plane_stride;   // out_w * out_h * 4 bytes, out_w * out_h elements
	double interval_m, base_m, exaggeration;
	double light[3];
	uint32_t mm[4];                      // per call: the minimap rectangle (valid iff has_mm)
	uint32_t out_w, out_h;
	uint32_t nearest;                    // SMHV_RELIEF_NEAREST
	uint32_t major_every;                // M
	uint32_t per_call, has_mm;           // 1: mm / has_mm are the call's and aux, res are not read
	uint32_t shade_weight;
	uint32_t pal[2];                     // contour, major: R, G, B, a as a little-endian word
	uint32_t pad;
};
// smhv_batch_scale_labels / smhv_scale_labels (k_scale_labels: smh_scalelabels.hip): the scale labels of n frames, one workgroup
// each.  Launch arguments, taken by value at the launch.
#define SMH_SL_MAX_DIM 2048u             // the quadrant's padded row and its height, at most: a row is two 16-byte loads per lane of a wave
struct ScaleLabelsRun {
	const FrameAux *aux;                 // per frame: open
	const uint8_t *ocr;                  // P: the ocr_preprocess slab at the first frame of the call (pixel x of a row at byte q_xoff + x)
	const uint8_t *s0;                   // S0: find_scales_preprocess with start row 0, the same layout
	smhv_scale_label_frame *out;         // the label slab, at the first frame of the call
	uint8_t *crops;                      // the crop slab: SMHV_LABEL_FRAME_CROP_BYTES per frame
	uint64_t stride;                     // bytes between two frames' planes
	uint32_t pitch, q_xoff, qw, qh;      // the planes' row pitch in bytes (a multiple of 64, at most SMH_SL_MAX_DIM), the quadrant
	uint32_t gap;                        // g
};
// smhv_batch_label_text / smhv_label_text (k_label_text: smh_labeltext.hip): the texts of n frames' scale labels, one workgroup each.
// Launch arguments, taken by value at the launch.
struct GlyphAtlas;                       // smh_glyph_rule.h
struct LabelTextRun {
	const smhv_scale_label_frame *labels; // the label slab, at the first frame of the call
	const uint8_t *crops;                // the crop slab: SMHV_LABEL_FRAME_CROP_BYTES per frame
	const GlyphAtlas *atlas;             // device
	smhv_label_text_frame *out;          // the text slab
	smhv_anchors *anchors;               // the frames' anchors, tightly packed
};
// smhv_batch_probe / smhv_batch_render_debug / smhv_render_map_debug (k_probe, k_debug_plan, k_debug_draw: smh_debugtext.hip): the
// vision debugger's numbers and the debug text of n frames.  Launch arguments, taken by value at the launch.
#define SMH_DBG_ITEMS (SMHV_TEXT_MAX_RUNS + 1u + 4u * SMHV_MAX_PROBES)   // a frame's item list: the runs, the caption, four per probe
#define SMH_DBG_TEXT 200u                // bytes of a probe's string in the plan's pool (197 at most, were every field at its type's limit)
#define SMH_DBG_NONE 0u                  // DebugItem::kind: nothing (an empty bounding box)
#define SMH_DBG_TEXT_ITEM 1u             //   a text run at anchor (ax, ay)
#define SMH_DBG_FILL 2u                  //   a fill of [a, b)
#define SMH_DBG_FRAME 3u                 //   the SMHV_PRIM_RECT rule on corners a, b
struct DebugItem {                       // 72 bytes; a fixed place in the frame's list per run, caption and probe part: paint order
	const uint8_t *text;                 // the run's bytes (the call's run list, the plan's pool or the caption)
	float ax, ay, bx, by;
	int32_t x0, y0, x1, y1;              // window bounding box, half-open, clamped to the window: a superset of what the rule paints
	uint32_t color;                      // RGBA8 as a little-endian word, alpha 255
	uint32_t kind;
	uint32_t n_lines, pad;
	uint8_t off[8], len[8];              // text: where each line starts in `text` and how many characters it has
};
struct DebugRun {
	const uint8_t *ui;                   // the ui slab, at the first frame of the call
	const FrameAux *aux;                 // per frame: open
	const smhv_frame_result *res;        // per frame: has_minimap
	const smhv_text_run *runs;           // device memory: the call's runs
	const smhv_probe_point *points;      // device memory: the call's probe points
	smhv_probe *probes;                  // the probe slab, at the first frame of the call: SMHV_MAX_PROBES per frame
	DebugItem *items;                    // SMH_DBG_ITEMS per frame, at the first frame of the call
	uint8_t *pool;                       // SMHV_MAX_PROBES * SMH_DBG_TEXT bytes per frame: the probes' strings
	uint8_t *img;                        // the render slab, at the first frame of the call (null: the probe alone)
	uint64_t img_stride;                 // out_w * out_h * 4
	uint32_t out_w, out_h;
	uint32_t n_runs, n_points;
	uint32_t flags;                      // SMHV_DEBUG_*
	uint32_t scale;                      // S, 1 .. 4
	float sw, sh, tx, ty;                // the viewport
};
// ---- the mask as the streaming passes leave it for the line search (round 6) -------------------------------------------------
// A marker mask is 1-4 % non-empty, and what the search keeps in LDS is its non-empty 32 x 8 px tiles.  Finding them in the
// row-major bit rows meant walking the bounding box of the set bits: (tile rows x tile columns) x 16 strided dword loads, ~68 KB
// and ~19 dependent round trips per 1080p frame, from one wave, while the streaming pass saturates the memory system.  The
// pass knows which tiles are empty when it writes them, so it also leaves
//   tiled  the bit rows tile-major: tile (ty, wx) = rows 8 ty .. 8 ty + 7 of word column wx of the bit-packed rows (Geom::bits_pitch_w
//          word columns; bit 0 of word column 0 is the ROI's quad-aligned x, m_xoff bits left of pixel 0), 8 consecutive words.
//          Only tiles with a set bit are written (by the wave that owns the word column in that band).
//   occ    one byte per (tile row, wave of the pass): bit j = tile (ty, 8 wave + j) holds a set bit.  Every band of an open frame
//          writes the bytes of its tile rows (zeros too), so nothing stale is ever read.
// The builder reads the occupancy bytes of the bounding box's tile rows (one coalesced load) and then exactly the non-empty
// tiles (32 contiguous bytes each, all in flight together): 2-3 round trips and 4-9 KB.  Bands have to be a multiple of 8 rows tall
// for this (24 rows up to 1080p, where short bands are also the faster ones; 56 instead of 58 above, 20 bands instead of 19 at 1440p): a
// launch takes them where they are free or pay (band_rows_for, smh_stream.hip) and says so per frame in FrameAux::tiles; otherwise the search walks the bit rows as before.
__host__ __device__ inline uint32_t tiled_rows(const Geom &g) { return (g.rh + 7u) >> 3; }
__host__ __device__ inline uint64_t tiled_stride_w(const Geom &g) { return (uint64_t)tiled_rows(g) * g.bits_pitch_w * 8u; }
__host__ __device__ inline uint32_t occ_pitch(const Geom &g) { return ((g.m_block >> 6) + 3u) & ~3u; }
__host__ __device__ inline uint64_t occ_stride(const Geom &g) { return (uint64_t)tiled_rows(g) * occ_pitch(g); }

#define SMH_RAY_OFF_BATCHES 168u     // 5376 steps: longer than the diagonal of the largest supported ROI (4096 x 3300)

// Sector culling table as k_build_sector_table writes it: (2R+1)^2 entries, entry (oy+R)*(2R+1) + (ox+R) = bit mask of the
// 64-ray units that can sample the pixel at offset (ox, oy) from floor(start point), and the annuli it lies in -- steps
// [50 - T, 50] and [50 - 2T - 1, 50 - T - 1] (smh_cull_rule.h: smh_cull_entry).  The host condenses it into the per-word
// cells of Buffers::cull_tab: one mask per annulus the build scans (SMH_CULL_ANNULI: the outer one; with -DSMH_CULL_CHAIN the
// middle one too), one unit code per pixel.
#include "smh_cull_rule.h"
#define SMH_SECTOR_R 52
#define SMH_SECTOR_DIM (2 * SMH_SECTOR_R + 1)
#define SMH_SECTOR_ENTRIES (SMH_SECTOR_DIM * SMH_SECTOR_DIM)
#define SMH_CULL_CELLS (SMH_SECTOR_DIM * 4)
#define SMH_CULL_TAB_WORDS (SMH_CULL_ANNULI * SMH_CULL_CELLS + (SMH_SECTOR_ENTRIES + 3) / 4)
#define SMH_CULL_CODES(tab) ((const uint8_t *)((tab) + SMH_CULL_ANNULI * SMH_CULL_CELLS))
#define SMH_CULL_MID_CELL(tab, cell) (SMH_CULL_ANNULI == 2 ? (tab)[(SMH_CULL_ANNULI - 1) * SMH_CULL_CELLS + (cell)] : 0u)   // (no middle mask in a build without the chain)

// ---- the frame-granular line search of a pipeline (k_lsd_service, smh_service.inc; round 4) -------------------------------
// A batch-granular search launch lasts as long as its slowest frame, and the slot cannot be resubmitted before.  A pipeline of
// depth >= 3 therefore runs ONE long-lived search kernel per device: its waves pull (slot, frame) items from a ring in device
// memory, search the frame (one wave per frame: the reference's sequential scan as it stands, smh_lsd_seq.inc), write the
// frame's record and count it off against its submission; the wave that finishes a submission's last frame stores the
// submission's sequence number into host-mapped memory, which is what smhv_pipeline_wait polls.  The streaming side of a
// submission ends with k_svc_publish, which writes the slot's descriptor and the items.
//   SvcSlot   per pipeline slot, device memory: what the waves need to know about the slot's current submission
//   SvcCtl    per pipeline, device memory: the ring and its counters
//   SvcHost   per pipeline, mapped host memory: life-cycle handshake and completion flags
// Life cycle: the kernel is launched by the submission that finds it not alive and closes ITSELF when every submitted
// batch is complete and nothing has arrived for `idle_short` cycles -- atomically with respect to the host's next submission
// (compare-and-swap on SvcHost::state, which names the launch that is alive), so a device-wide synchronize by anybody still
// returns.
#define SVC_MAX_SLOTS 32u
struct SvcSlot {
	Buffers b;                          // the submission's buffers, record stages, anchors, ... (as the batch kernels get them)
	uint32_t n;                         // frames of the submission
	uint32_t seq;                       // its sequence number (never 0)
	uint32_t done;                      // frames finished so far
	uint32_t pad;
	unsigned long long t_pub;           // s_memrealtime (100 MHz) when the items were published (diagnostics: where a submission's time goes)
};
// ---- help across workgroups (round 5) -----------------------------------------------------------------------------------------
// The help desk of smh_lsd_seq.inc lives in the owner's LDS: only the waves of its workgroup (three or four) can serve it, and a
// frame with several hundred rounds still takes milliseconds -- long enough to block its submission's slot.  A frame that has
// been at work for SvcParams::remote_after rounds therefore also asks the waves of OTHER workgroups: it writes its tile store
// (the mask as it holds it in LDS: the non-empty tiles + the 16-bit index) into its own block of SvcParams::remote_store,
// opens its SvcRemote and puts `tickets` into the service's help ring; a wave between two frames of its own that pops a
// ticket attaches (compare-and-swap on SvcRemote::state), copies the store into its own LDS block and casts the candidates the
// owner posts in SvcRemote::ring -- exactly what a helper of the owner's workgroup does through LDS, with 8-byte agent-scope
// granules in global memory instead.  The owner matches results to pixels and visits the scan's pixels in the scan's order:
// lines, rounds and sample counts are the sequential reference's whoever cast what (a cast is a pure function of mask and pixel).
#define SVC_REMOTE_RING 12u             // posts a frame may have out to helpers of other workgroups
#define SVC_REMOTE_OPEN 0x80000000ull
struct SvcRemoteEntry {                 // 64 bytes
	unsigned long long post;            // owner -> helpers: k32 << 32 | py16 << 16 | px16 (k = 1, 2, ...: the request's posts in order; 0 = none); one 8-byte agent-scope granule
	unsigned long long claim;           // the highest k anybody has taken (atomic max: a helper to cast it, or the owner taking it back)
	// helper -> owner: the result as two 16-byte granules, each written by ONE write-through store and read by ONE 16-byte load,
	// each carrying the post's number -- a half is valid when its k is the one waited for, whatever the order the two arrive in
	// (one round trip for the owner instead of tag-then-payload):
	uint32_t res_a[4];                  //   k, mask samples, len^2 bits of the longest exactly evaluated ray (0: none), its ray index
	uint32_t res_b[4];                  //   k, ex bits, ey bits (that ray's end point), start point: (2 pty)16 << 16 | (2 ptx)16 (get_centre yields multiples of 0.5)
	unsigned long long pad[2];
};
struct SvcRemote {                      // one per wave of the service launch (owner = workgroup * waves + wave)
	unsigned long long state;           // request number32 << 32 | SVC_REMOTE_OPEN | helpers attached
	unsigned long long info;            // non-empty tiles of the frame's store (what a helper has to copy), written before the request opens
	unsigned long long pad[6];
	SvcRemoteEntry ring[SVC_REMOTE_RING];
};
#define SVC_HELP_RING 256u              // tickets in flight (a power of two)
struct SvcCtl {
	// (avail and closing are what an idle wave looks at: one 8-byte load.  Every idle wave of the chip polls this one address,
	// i.e. one memory channel: smh_service.inc spaces the polls out -- at 2 us per wave the streaming pass beside them took 1.6 ms
	// instead of 0.9: a pass is as slow as its slowest channel)
	int32_t avail;                      // items published and not yet claimed (semaphore; transiently negative)
	uint32_t closing;                   // epoch of the service launch that has closed
	int32_t help_avail;                 // help tickets nobody has taken (semaphore): the second word of an idle wave's look
	uint32_t help_head, help_reserve;   // help tickets handed out / reserved by owners
	uint32_t stat_remote;               // diagnostics: candidates cast for frames of other workgroups
	uint32_t head;                      // tickets handed out
	uint32_t reserve;                   // ring entries reserved by publishers
	uint32_t completed;                 // submissions finished (counts like SvcHost::state >> 1)
	uint32_t busy;                      // waves working on a frame
	uint32_t stat_items, stat_waves;    // diagnostics (smhv_debug_pipeline_stats): frames searched; waves that have come and gone
	unsigned long long stat_busy, stat_life;   // cycles spent on frames / between a wave's first poll and its exit, summed over those waves
	unsigned long long stat_phase[4];   // of stat_busy: acquire (cache invalidation), tile store + search, record (scale ratio + derived outputs), release + count
	unsigned long long stat_help;       // cycles spent casting candidates for other waves' frames (not in stat_busy)
	uint32_t stat_requests, stat_attached;   // help requests opened across workgroups; helpers that attached to one
	// where a submission's time goes, in ticks of s_memrealtime (100 MHz), summed: publication -> a wave takes the frame (per frame);
	// publication -> the submission's last frame is counted off (per submission); how long that last frame itself was at work
	unsigned long long stat_t_wait, stat_t_sub, stat_t_last;
	// helpers of other workgroups' frames: polls of a request's ring, polls that found nothing to take, claims lost to somebody quicker, exits because
	// nothing came / the request closed, cycles attached
	uint32_t stat_h_polls, stat_h_empty, stat_h_lost, stat_h_idle_exit, stat_h_closed_exit, stat_h_pad;
	unsigned long long stat_h_cycles, stat_h_cast_cycles;
	unsigned long long help_ring[SVC_HELP_RING];   // ticket gen32 << 32 | request number16 << 16 | owner16
	// (the item ring is an allocation of its own: gen32 << 32 | slot << 24 | frame, gen = (ticket >> log2 cap) + 1)
};
struct SvcHost {
	// submissions so far << 32 | epoch of the service launch that is alive (0: none).  The host adds submissions and -- only
	// when it finds the low half 0 -- puts a new launch's epoch there; only waves of THAT launch clear it again (64-bit
	// compare-and-swap over PCIe), and a wave that finds another launch's epoch (or none) there leaves: no launch can outlive
	// its own entry, whatever the interleaving.
	unsigned long long state;
	uint32_t launches;                  // service launches so far (diagnostic)
	uint32_t pad0;
	uint32_t done_seq[SVC_MAX_SLOTS];   // per slot: sequence number of its last completed submission
	uint32_t pad[12];
};
struct SvcParams {
	SvcCtl *ctl;
	unsigned long long *ring;
	SvcSlot *slots;
	SvcHost *host;                      // device address of the mapped host block
	const uint32_t *cull_tab;           // the sector table every submission of this launch uses (null: every ray is cast)
	const float *ray_off;               // Buffers::ray_off of the context (the same for every slot)
	float max_gap;
	uint32_t tile_cap, list_cap;        // per-wave tile store and list sizes
	uint32_t part_words;                // LDS words per wave (WShared + tile store + lists + window)
	uint32_t ring_log2;
	uint32_t epoch;                     // of this launch (> 0)
	uint32_t idle_short, idle_long;     // in units of 1024 cycles
	uint32_t flags;                     // experiments (SMH_SVC_FLAGS; results may be WRONG): 1 = no cache invalidation per item, 2 = no write-back per frame, 4 = s_setprio 3, 8 = no helping among the waves of a workgroup
	                                    // 32 = the tile store is built by walking the bit rows' bounding box (rounds 2-5) instead of from the pass's tile-major mask (A/B)
	// help across workgroups (null / 0: none)
	SvcRemote *remote;                  // one per wave of the launch
	uint32_t *remote_store;             // owner o's tile store: remote_store + o * remote_store_words
	uint32_t remote_store_words;
	uint32_t remote_after;              // rounds a frame works (with its workgroup's help) before it asks the other workgroups
	uint32_t remote_tickets;            // helpers it asks for
	uint32_t remote_last_div;           // ... once it is among the last 1 / remote_last_div of its submission's frames still at work
	uint32_t compact;                   // the waves' tile stores sit behind the compact index (LSD_MODE_TILEC): decided by svc_waves_for for the frame size
	// (flags & 16: frames ask, and waves take tickets, whether or not frames are waiting for a wave -- A/B)
};
// waves per service workgroup and LDS per workgroup for this frame size (0 waves: the frame size does not fit -> no service)
// (*compact <- whether the tile stores use the compact index: where that lets one more wave fit)
uint32_t svc_waves_for(const Geom &g, uint32_t tile_limit, uint32_t *part_words, uint32_t *tile_cap, uint32_t *list_cap, uint32_t *lds_bytes, uint32_t *compact = nullptr);
uint32_t svc_store_words_for(const Geom &g, uint32_t tile_cap, uint32_t compact);   // words of a frame's tile store (tiles + index), rounded up to whole 16-byte quads
hipError_t svc_probe_host_atomics(SvcHost *h, SvcHost *d_h, bool *ok);   // pipeline creation: do device-side system-scope atomics reach mapped host memory?
hipError_t launch_svc_publish(SvcCtl *ctl, unsigned long long *ring, SvcSlot *slots, uint32_t slot, const Buffers &b, uint32_t n, uint32_t seq, uint32_t ring_log2, hipStream_t s);
hipError_t launch_lsd_service(const Geom &g, const SvcParams &p, uint32_t workgroups, uint32_t waves, uint32_t lds_bytes, hipStream_t s);

enum : uint32_t { MAP_UI = 1u, MAP_MASK = 2u, MAP_BYTES = 4u, MAP_PRIO = 0x100u, MAP_BAND_MAJOR = 0x200u };   // MAP_BAND_MAJOR: the order of the work items (launch_map_brq_pass)
// MAP_BYTES (k_map_pass only): the pass also writes the mask one byte per pixel (Buffers::mask) -- the per-call path, whose mask goes
// straight to the host.  Batch runs leave it out: their passes write the bit rows (and the tile-major mask), and the byte form is
// made from the bit rows when a reader asks for it (launch_mask_expand; smh_runtime.cpp, batch_materialize_mask).
enum : uint32_t { BRQ_OCR = 1u, BRQ_SCALES = 2u };

// ---- the grey ui_map as a luma plane ------------------------------------------------------------------------------------------
// A grey ui_map is (l,l,l,255): three of every four bytes repeat a byte the pass also writes.  A grey batch run therefore writes
// one byte per pixel into a plane of its own -- the ui slab's quads, rows and frames at a quarter of the pitch and stride -- and
// the RGBA slab is made from it when a reader asks (launch_ui_expand; smh_runtime.cpp, batch_materialize_ui), as the byte mask is
// made from the bit rows.  Unlike the mask the slab has two writers (colour runs, overlay runs and the runs of a batch whose caller
// holds the slab write RGBA directly) and a frame a run finds closed keeps its older image, so ONE persistent byte per frame says
// where a frame's newest ui_map lies: UI_FORM_LUMA the plane, UI_FORM_RGBA the slab.  k_button writes it for the open frames of a
// run with the ui stage; k_ui_expand expands exactly the flagged frames and the flags are cleared behind it.
// The passes take the plane where they take the slab: Buffers::ui = the plane and `grayscale` = 2.
enum : uint32_t { UI_FORM_RGBA = 0u, UI_FORM_LUMA = 1u, UI_FORM_KEEP = 2u };
hipError_t launch_button(const Geom &g, const Buffers &b, uint32_t n, int force_open, hipStream_t s, uint8_t *ui_form = nullptr, uint32_t ui_luma = UI_FORM_KEEP);
// frames [0, n): where ui_form[f] == UI_FORM_LUMA, the frame's RGBA rows (d_ui) from its luma plane (d_luma); clears those flags behind it
hipError_t launch_ui_expand(const Geom &g, const uint8_t *d_luma, uint8_t *d_ui, uint8_t *ui_form, uint32_t n, hipStream_t s);
// grayscale: 0 = colour, 1 = (l,l,l,255), 2 = the luma plane (b.ui = the plane; not with MAP_BYTES)
// tiles_wanted: the batch path (the mask also tile-major where the bands allow it: band_rows_for); the per-call path leaves it
hipError_t launch_map_pass(const Geom &g, const Buffers &b, uint32_t n, uint32_t flags, int grayscale, hipStream_t s, bool tiles_wanted = false, bool overlapped = false);
// map pass + quadrant pass in one (the quadrant pixels are read once); flags: MAP_*, qflags: BRQ_*
// Occupancy policy of a pipelined batch (smhv_pipeline_create).  A streaming workgroup beyond the two per
// CU that saturate HBM only waits in the memory queues -- while holding wave slots and registers the other batches' line
// searches need -- so the pipeline (a) makes every streaming workgroup reserve enough LDS that a third does not fit on a
// CU and a line-search workgroup still does, and (b) caps the streaming grid (workgroups walk the (frame, band) items with
// a grid stride).  All zero: no policy (a batch that runs alone).
struct LaunchTuning {
	uint32_t map_lds_total;   // LDS a streaming workgroup occupies, static + dynamic, in bytes (0: what it needs)
	uint32_t map_grid_cap;    // streaming workgroups per launch (0: one per item)
	uint32_t lsd_tile_limit;  // k_lsd_tile keeps at most this many mask tiles in LDS (0: what fits the kernel's own budget)
	uint32_t map_prio;        // != 0: the streaming waves run at wave priority 3 -- ahead of the search service's waves on their SIMD,
	                          // which have slack (measured: 470 k -> 516 k frames/s at depth 12; beside the batch-granular search it cost 1-8 %)
	uint32_t map_deep;        // != 0: three register sets of loads in flight per wave instead of two (launch_map_brq_pass)
	uint32_t map_overlapped;  // != 0: the launch overlaps other kernels of its pipeline (the search service, or the searches and passes of a batch-granular
	                          // pipeline of depth >= 3): 56-row bands up to 1080p and frame-major work items, where a launch that runs ALONE (plain
	                          // runs, the per-call path, pipelines of depth 1 and 2) takes 24-row bands in band-major order (band_rows_for, k_map_brq_pass)
};
// LDS of one workgroup of the fused streaming pass without a reservation / of k_lsd_tile with `tile_cap` tiles (static + dynamic)
uint32_t map_brq_lds_bytes(const Geom &g);
uint32_t lsd_tile_lds_bytes(const Geom &g, uint32_t tile_limit);
hipError_t launch_map_brq_pass(const Geom &g, const Buffers &b, uint32_t n, uint32_t flags, uint32_t qflags, int grayscale, uint32_t fixed_start_y, int use_anchor_start, hipStream_t s,
                               const LaunchTuning *tune = nullptr);
// the fused streaming pass's loads and stores without its arithmetic (calibration: smhv_debug_pattern_copy)
hipError_t launch_pattern_copy(const Geom &g, const Buffers &b, uint32_t n, uint32_t rows_in_flight, hipStream_t s);
void map_band_rows(uint32_t rh, uint32_t n, int fused, uint32_t *rows, int *tiles);
hipError_t launch_brq_pass(const Geom &g, const Buffers &b, uint32_t n, uint32_t flags, uint32_t fixed_start_y, int use_anchor_start, hipStream_t s);
// k_lsd is three kernels, one per mask residency mode, each over all frames (a workgroup whose frame needs another mode
// exits at once).  When the whole ROI fits the LDS window (<= 1080p) every frame is a ROWS frame and only that kernel is
// launched; otherwise the three run concurrently on s, fk->s1 and fk->s2 (fork / join with the events), or back to back
// on s when fk is null.
struct LsdFork { hipStream_t s1, s2; hipEvent_t fork, join1, join2; };
bool lsd_rows_only(const Geom &g);   // every frame of this size is a ROWS frame: find_lines launches one kernel
// mode 0: find_lines (whole frame); mode 1: one find_longest_line round from (px,py), result in results[f].lines[0], len^2 in length_px[0]
// b.co (if present) is zeroed on `s` before the launch; extra_helpers: additional workgroups that only help (small batches).
// find_lines runs on k_lsd_tile unless the buffers carry the helper scheme (b.co), prefer_classic is set (the schedule knows
// better: smhv_pipeline at depth 2 on frames up to 1080p) or the process-wide diagnostic switch is.
// tile_bs: threads per workgroup of k_lsd_tile (0: 512; a batch that runs alone takes 1024)
// record_fused (optional) <- whether the launch writes the frames' records itself (b.rec_stages has SMH_REC_ON and the kernel
// picked is k_lsd_tile); otherwise the caller launches the record kernel behind it
hipError_t launch_lsd(const Geom &g, const Buffers &b, uint32_t n, float max_gap, int mode, float px, float py, hipStream_t s, const LsdFork *fk, uint32_t tile_bs = 0,
                      bool prefer_classic = false, uint32_t tile_limit = 0, bool *record_fused = nullptr);
size_t lsd_coop_ctl_bytes(uint32_t n);      // LsdCtl + n LsdCoop (one allocation, zeroed per launch)
hipError_t launch_scale_ratio(const Geom &g, const Buffers &b, uint32_t n, uint32_t *d_bars, hipStream_t s);
hipError_t launch_find_minimap(const Geom &g, const Buffers &b, uint32_t n, hipStream_t s);
hipError_t launch_finalize(const Geom &g, const Buffers &b, uint32_t n, uint32_t stages, hipStream_t s);
hipError_t launch_scales_finalize(const Geom &g, const Buffers &b, uint32_t n, uint32_t stages, uint32_t *d_bars, hipStream_t s);   // scale ratio + finalize
// firing solutions (smh_firing.h): explicit lines (smhv_firing_solutions), and the heightmap colour map's two passes
// (mm: two words, {max, min}, initialised to {0, 0xFFFFFFFF} on `s` by the launcher)
hipError_t launch_firing_lines(const FiringRun &r, const smhv_line *lines, uint32_t n, uint32_t has_mpx, double mpx, uint32_t has_minimap,
                               const uint32_t minimap[4], smhv_firing *out, hipStream_t s);
hipError_t launch_heightmap_color_map(const uint16_t *hm, uint64_t n, uint32_t *mm, uint32_t *rgba, hipStream_t s);
// the overlay: the colour table of a heightmap (lut: 65,536 words; mm as above), and the composite over n frames of a slab
#define SMH_HM_LUT_ENTRIES 65536u
hipError_t launch_heightmap_lut(const uint16_t *hm, uint64_t n, uint32_t *mm, uint32_t *lut, hipStream_t s);
hipError_t launch_hm_overlay(const Geom &g, const OverlayRun &r, uint32_t n, hipStream_t s);
// the map view (smh_render.hip).  render_set_form: 0 = the launcher's rule, 1 = gathers, 2 = LDS staging, 3 = the colour table in LDS (smhv_debug_render_form);
// render_rule: the form the rule takes for a call (2 or 3), *texels <- the LDS texels of the staged form (the footprint of one band
// of a tile), *ratio <- heightmap texels per output pixel; render_switch_ratio: the ratio up to which the rule stages
hipError_t launch_render_map(const Geom &g, const RenderRun &r, uint32_t n, hipStream_t s);
// the same with layers: k_render_map_layers of the form the same rule (or smhv_debug_render_form) takes
hipError_t launch_render_map_layers(const Geom &g, const RenderRun &r, const RenderLayersRun &y, uint32_t n, hipStream_t s);
// the 16-bit form of a heightmap's colour table: lut16 = SMH_HM_LUT_ENTRIES halfwords, *vr = the lowest value with red in its colour
hipError_t launch_heightmap_lut16(const uint32_t *lut, uint16_t *lut16, uint32_t *vr, hipStream_t s);
#define SMH_HM_LUT_WORDS (SMH_HM_LUT_ENTRIES + 4u + SMH_HM_LUT_ENTRIES / 2u)   // 32-bit table, {max, min, vr, -}, 16-bit table
// the marker labels (smh_labels.hip): k_label_plan over n frames, then k_label_draw over their images
hipError_t launch_labels(const LabelRun &r, uint32_t n, hipStream_t s);
// the reach map (smh_reach.hip): k_reach<paint, classes> over n frames (at most 65,535: the grid's third dimension)
hipError_t launch_reach(const ReachRun &r, uint32_t n, bool paint, bool classes, hipStream_t s);
// the terrain relief (smh_relief.hip): k_relief<paint, planes> over n frames (at most 65,535), then k_relief_finish over their
// summaries; the planes asked for are the non-null pointers of r
hipError_t launch_relief(const ReliefRun &r, uint32_t n, bool paint, hipStream_t s);
// terrain clearance (smh_clear.hip): k_clear_lines over n frames x SMHV_MAX_LINES lines (per call: n = 1, r.n_lines lines), and
// k_clear_map<paint, bytes> over n frames (at most 65,535 each: a grid dimension)
hipError_t launch_clear_lines(const ClearLinesRun &r, uint32_t n, hipStream_t s);
hipError_t launch_clear_map(const ClearMapRun &r, uint32_t n, bool paint, bool bytes, hipStream_t s);
// scale labels (smh_scalelabels.hip): k_scale_labels over n frames; gap: the rule's g for a quadrant qw wide (host)
hipError_t launch_scale_labels(const ScaleLabelsRun &r, uint32_t n, hipStream_t s);
uint32_t scale_labels_gap(uint32_t qw);
// scale labels: text (smh_labeltext.hip): k_label_text over n frames
hipError_t launch_label_text(const LabelTextRun &r, uint32_t n, hipStream_t s);
// the vision debugger and the debug text (smh_debugtext.hip): k_probe over n frames; with r.img also k_debug_plan and k_debug_draw
hipError_t launch_debug_text(const Geom &g, const DebugRun &r, uint32_t n, hipStream_t s);
void render_set_form(uint32_t form);
uint32_t render_rule(const Geom &g, const RenderRun &r, uint32_t *texels, float *ratio);
float render_switch_ratio();
// which: SMHV_VIEW_*; isolated: LSDPreprocess shows the marker-isolated crop (after isolate_map_markers)
hipError_t launch_debug_view(const Geom &g, const Buffers &b, uint32_t frame, int which, int isolated, uint8_t *d_rgba, hipStream_t s);
hipError_t launch_marker_table(uint32_t *d_bits, hipStream_t s);
// the marker mask one byte per pixel (Buffers::mask) of frames [0, n) from their bit rows (Buffers::bits): byte x of a row = 0xFF where bit x of the
// row is set, the padded row width (mask_pitch bytes) for rows 0 .. rh - 1
hipError_t launch_mask_expand(const Geom &g, const uint32_t *d_bits, uint8_t *d_mask, uint32_t n, hipStream_t s);
hipError_t launch_pack_rows(const void *d_src, uint32_t src_pitch_bytes, void *d_dst, uint32_t row_bytes, uint32_t rows, hipStream_t s);   // pitched rows -> a tight buffer (dword granularity)
hipError_t launch_side_probe(uint32_t *d_out, uint32_t workgroups, uint32_t spin, hipStream_t s);   // a 21 KB-LDS / 280-VGPR kernel that does nothing (co-residency probe)
hipError_t launch_build_sector_table(unsigned long long *d_tab, uint32_t T, hipStream_t s);
hipError_t launch_build_ray_offsets(float *d_off, hipStream_t s);   // 3600 x (SMH_RAY_OFF_BATCHES + 1) float2
size_t lsd_lds_bytes();
// diagnostic: find_lines on the workgroup-synchronous k_lsd for every frame instead of k_lsd_tile 
void lsd_set_classic(bool on);
// diagnostic: cap the tile store of k_lsd_tile (0 = what fits), to exercise the path of frames with more tiles than that
void lsd_set_tile_cap(uint32_t cap);
// diagnostic: threads per workgroup of every k_lsd_tile launch (0 = the caller's choice; 128 .. 1024)
void lsd_set_threads(uint32_t threads);
// diagnostic: watchdog budget of k_lsd_tile in idle polls (0 = default)
void lsd_set_spin_limit(uint32_t polls);
// overwrite the 3600 ray directions of the current device's code object (synchronous)
hipError_t set_ray_table(const float *dx, const float *dy);
// CRC-32 of n_dwords 32-bit words at d_msg, xor-ed into *d_acc (zero it first) WITHOUT the init / final-xor terms:
//   crc = *d_acc ^ crc32_mul(crc32_xpow(32 * n_dwords), 0xFFFFFFFF) ^ 0xFFFFFFFF.
// wgs workgroups of SMH_CRC_BS threads, rounds * wgs * SMH_CRC_BS * 4 >= n_dwords; x_skip = x^(128 (G - 1)),
// d_x_local[t] = x^(128 (SMH_CRC_BS - 1 - t)), d_x_wg[g] = x^(128 SMH_CRC_BS (wgs - 1 - g)), G = wgs * SMH_CRC_BS.
#define SMH_CRC_BS 1024
// decoder layouts -> BGRA8 (n_px pixels; layout = SMHV_PIXELS_*)
hipError_t launch_to_bgra(const void *d_src, void *d_bgra, uint64_t n_px, uint32_t layout, hipStream_t s);
// ---- 4:2:0 video frames -> BGRA8 (smh_yuv.hip; smhv_yuv_to_bgra_device and the ingest queue) ------------------------------
#define SMH_YUV_NV12 5                       // == SMHV_PIXELS_NV12 / _I420
#define SMH_YUV_I420 6
#define SMH_YUV_BAND_PAIRS 4u                // row pairs of a workgroup's band
struct YuvCoef { int cy, yoff, rv, gu, gv, bu; };   // a row of the header's table
// A rectangle of the frame to convert and where its samples lie, as byte offsets from the frame's source base: the Y sample of
// frame pixel (y_x0, y_y0) at y_off, rows y_pitch apart; the chroma sample (c_x0, c_y0) at u_off / v_off (NV12: the pair at
// u_off), rows uv_pitch apart.  y_x0 <= x0 & ~3 and c_x0 <= (x0 & ~3) / 2; for the bilinear form the chroma rows and columns
// reach one sample beyond what the rectangle's pixels lie in (clamped at the frame's edge).
struct YuvRect {
	uint32_t x0, y0, w, h;
	uint64_t y_off, u_off, v_off;
	uint32_t y_pitch, uv_pitch, y_x0, y_y0, c_x0, c_y0;
};
struct YuvRun {
	const uint8_t *src; uint8_t *dst;        // first frame; frames src_stride / dst_stride bytes apart, output rows W * 4 bytes
	uint64_t src_stride, dst_stride;
	uint32_t W, H, n;
	uint32_t bands0, bands_total;            // (filled in by the launcher)
	YuvCoef k;
	YuvRect r[2];
};
hipError_t launch_yuv_to_bgra(YuvRun run, uint32_t n_rects, uint32_t layout, uint32_t bilinear, hipStream_t s);
// ---- RGBA8 / BGRA8 / luma images -> 4:2:0 video frames (smh_yuvout.hip; smhv_bgra_to_yuv_device, smhv_batch_video) -----------
struct YuvOutCoef { int yr, yg, yb, yoff, ur, ug, ub, vr, vg, vb; };   // a row of the header's outbound table
// n images of w x h.  A frame is read from ONE of two sources: its pixels (src: 4 bytes each, 4-byte aligned, rows src_pitch and
// images src_stride apart, both multiples of 4) or its luma plane (luma: one byte per pixel, rows luma_pitch and images luma_stride
// apart, any byte alignment; the kernel reads the aligned dwords its bytes lie in, so the allocation begins and ends on a 4-byte
// boundary, as the batch's plane does).
// form: null = every frame from src (or from luma where src is null); else frame f from luma where form[f] == UI_FORM_LUMA.
// dst: frames dst_stride apart, Y rows y_pitch apart from offset 0, chroma rows uv_pitch apart at u_off / v_off (NV12: the pairs
// at u_off), any byte alignment.
struct YuvOutRun {
	const uint8_t *src, *luma, *form;
	uint8_t *dst;
	uint64_t src_pitch, src_stride, luma_pitch, luma_stride;
	uint64_t y_pitch, uv_pitch, u_off, v_off, dst_stride;
	uint32_t w, h, n, rgba;                  // rgba: the pixels' bytes are R, G, B, A (0: B, G, R, A)
	uint32_t groups, pairs, items;           // (filled in by the launcher: columns of 8 pixels, row pairs, n * pairs * groups)
	YuvOutCoef k;
};
hipError_t launch_bgra_to_yuv(YuvOutRun run, uint32_t layout, hipStream_t s);
hipError_t launch_unpack_rows(const void *d_pack, void *d_frame, uint32_t pitch_px, uint32_t roi_x, uint32_t roi_y, uint32_t roi_w, uint32_t roi_h, uint32_t btn_x,
                              uint32_t btn_y, uint32_t btn_w, uint32_t btn_h, hipStream_t s);
hipError_t launch_crc32(const void *d_msg, uint64_t n_dwords, uint32_t wgs, uint32_t rounds, uint32_t x_skip, const uint32_t *d_x_local,
                        const uint32_t *d_x_wg, uint32_t *d_acc, hipStream_t s);
uint32_t crc32_xpow(uint64_t n);                 // x^n mod P (reflected representation, x^0 = 0x80000000)
uint32_t crc32_mul(uint32_t a, uint32_t b);      // a * b mod P

// ---- the remote-viewer feed (smh_feed.hip; smhv_batch_feed / smhv_feed_frame) -------------------------------------------------
// Launch arguments of a feed call over n frames, taken by value at the launch.  Everything a frame index applies to (ui, res, raw)
// points at the call's first frame.
struct FeedMap { uint64_t dst; uint32_t frame, pad; };   // a Map entry of the call: payload offset in the buffer, frame (index in the call)
struct FeedRun {
	const uint8_t *ui;                   // the ui slab
	const smhv_frame_result *res;        // the records: map_open, status, mpx, minimap, lines
	uint64_t ui_stride, ui_pitch;
	uint32_t w, h, xoff, quads;          // the map; ROI pixel 0 sits xoff pixels into a slab row; 16-byte groups of a slab row that hold map bytes
	uint32_t n, first, flags;            // frames of the call, the batch index of the first (for the entries), SMHV_FEED_*
	uint32_t len_term;                   // the init / final-xor term of a CRC-32 over w h 4 bytes
	uint32_t rows_per_wave;              // of k_map_crc (feed_rows_per_wave)
	uint64_t capacity;                   // bytes of the message buffer
	uint32_t *raw;                       // n words: the frames' CRCs without that term (zeroed by the launcher)
	const uint32_t *tab;                 // k_feed_tables for (w, h, xoff): quads + h words
	uint32_t *state;                     // {has, crc}: the stored CRC
	smhv_feed_header *header;
	smhv_feed_entry *entries;            // 3 n
	uint8_t *bytes;
	FeedMap *maps;                       // n
};
#define SMH_FEED_MAX_ROWS 16384u         // rows of a ui_map a feed's tables hold (a slab row has at most 1024 groups: compute_geom)
hipError_t launch_feed_tables(uint32_t *d_tab, uint32_t w, uint32_t h, uint32_t xoff, uint32_t quads, hipStream_t s);
uint32_t feed_rows_per_wave(uint32_t h, uint32_t n);
void feed_set_rows(uint32_t rows);   // diagnostic: rows per wave of every k_map_crc launch (0 = the rule)
hipError_t launch_feed(const FeedRun &r, hipStream_t s);   // CRC, plan, compacting copy
// A debug view as the Map (smhv_batch_feed_view / smhv_feed_frame_view).  launch_feed_view: the same three steps over a message
// GENERATED from the source the FeedRun describes (src_mode = SMH_RND_SRC_GRAY / PREPROCESS / CROPPED; smh_feed.hip says what
// ui, ui_pitch, ui_stride, w, h, xoff and quads mean for each); its tables come from launch_feed_view_tables with ppg = 16 message
// dwords per 16-byte group for a plane, 4 for the colour sources (= launch_feed_tables).  launch_feed_image: one tight RGBA8
// image (the per-call path's materialised view) -- `crc` describes it to k_map_crc, `r` to the plan and the copy.
#define SMH_FEED_IMAGE_ROW 1024u         // dwords per row of launch_feed_image's description of a tight image
hipError_t launch_feed_view_tables(uint32_t *d_tab, uint32_t w, uint32_t h, uint32_t xoff, uint32_t quads, uint32_t ppg, hipStream_t s);
hipError_t launch_feed_view(const FeedRun &r, uint32_t src_mode, hipStream_t s);
hipError_t launch_feed_image(const FeedRun &crc, const FeedRun &r, hipStream_t s);
void feed_set_gray_form(uint32_t form);   // diagnostic: 0 = the rule, 4 = a plane's CRC with four lookups per message dword always

// ---- the feed's map tiles (smh_feedtiles.hip; smhv_batch_feed_tiles / smhv_feed_frame_tiles; the rule: smh_maptiles.h) --------------
// k_map_crc (smh_feed.hip) runs as it is; behind it, on the same stream and with no host round trip:
//   k_tiles_base   every frame's base: the nearest earlier open frame of the call, the feed's kept map, or none
//   k_tiles_diff   one bit per tile of every open frame that differs from its base, read where both maps lie
//   k_tiles_plan   k_feed_plan's scans, capacity cut and frames_done with a Map slot whose size and kind differ per frame
//   k_tiles_copy   persistent workgroups over (MapTiles message, 32 tiles): the index list and the padded tiles
//   k_feed_maps    (smh_feed.hip, as it is) the full Maps of the same call
//   k_tiles_keep   the last consumed open frame's map and CRC into the feed
__global__ void k_map_crc(FeedRun r);
__global__ void k_feed_maps(FeedRun r);
#define SMH_TILES_BASE_NONE 0xFFFFFFFFu  // a frame's base: none (it can only send a Map or nothing)
#define SMH_TILES_BASE_KEPT 0xFFFFFFFEu  // ... the feed's kept map; anything else: the index of a frame of the call
struct FeedTileItem { uint64_t dst; uint32_t frame, n; };   // a MapTiles message of the call: its offset in the buffer, frame (index in the call), tiles
struct FeedTilesRun {
	FeedRun r;                           // the call as smhv_batch_feed would make it (flags 0)
	uint8_t *kept;                       // the kept map: w x h RGBA, tightly packed
	uint32_t *kstate;                    // {valid, crc, w, h} of the kept map
	uint32_t *ctl;                       // {MapTiles messages of the call, the frame to keep (SMH_TILES_BASE_NONE: none), its CRC}
	uint32_t *base;                      // n: SMH_TILES_BASE_* or a frame of the call
	uint32_t *info;                      // 2 n: per frame the tiles that differ and the sum of their padded bytes (zeroed by the launcher)
	uint2 *bits;                         // n x words: per 32 tiles {the bits, the padded bytes of the set ones}
	FeedTileItem *items;                 // n
	uint32_t words;                      // 32-tile words of a frame's bitmap
};
hipError_t launch_feed_tiles(const FeedTilesRun &t, hipStream_t s);

}  // namespace smh
