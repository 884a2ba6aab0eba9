/*
 * smh_vision_hip.h -- C ABI of libsmh_vision_hip.so, the MI355X (gfx950) back-end for the
 * squad-mortar-helper vision hot path.
 *
 * This is the drop-in boundary: one function per method of the reference's plugin trait
 * `vision-common::Vision` (reference vision-common/src/lib.rs:30-61), i.e. exactly the table the
 * reference resolves from its GPU plugin dylib (`{name}_init`, `{name}_shutdown`,
 * `{name}_{load_frame,thread_ctx,crop_to_map,...}`; vision-common/src/dylib.rs:15-27,125-150).
 * The reference's own table is `extern "Rust"` (unstable ABI), so a ~150-line Rust shim crate
 * forwards each trait method to the function below (INTEGRATION.md shows it).  Plain pointers and
 * sizes only; every function returns 0 on success or a negative SMHV_E_* code and never throws or
 * aborts across the boundary (reference: Result<T, anyhow::Error>, vision-gpu/src/lib.rs:148).
 *
 * Parity target is the reference's CPU back-end (vision-cpu/src/lib.rs), NOT its CUDA back-end
 * (the two differ: SURVEY.md Appendix A).
 */
#ifndef SMH_VISION_HIP_H
#define SMH_VISION_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMHV_API __attribute__((visibility("default")))

/* error codes (negative).  smhv_last_error() returns the message of the calling thread's last failure. */
#define SMHV_OK 0
#define SMHV_E_INVALID (-1)  /* bad argument / call order (e.g. crop_to_map before load_frame)        */
#define SMHV_E_GEOMETRY (-2) /* frame size for which the reference's bounds arithmetic would panic    */
#define SMHV_E_HIP (-3)      /* HIP runtime error (message carries hipGetErrorString)                 */
#define SMHV_E_NO_DEVICE (-4)/* no usable gfx950 device -- the caller falls back to its CPU back-end
                                exactly as the reference does (src/vision/hardware.rs:73-76)          */
#define SMHV_E_STATE (-5)    /* map closed / stage output not available                               */

#define SMHV_MAX_LINES 32   /* find_lines::<32>, vision-common/src/lib.rs:58 */
#define SMHV_MAX_SCALES 3   /* src/vision/mod.rs:131 */

typedef struct smhv_ctx smhv_ctx;     /* one per device; ~ CudaInstance (vision-gpu/src/cuda.rs:15-94) */
typedef struct smhv_batch smhv_batch; /* resident frame batch + its output buffers                    */

/* == util::geometry::Line<f32> #[repr(C)] (util/src/geometry.rs:169-180): p0.x p0.y p1.x p1.y */
typedef struct { float x0, y0, x1, y1; } smhv_line;

/* log sink ~ the `&'static dyn log::Log` the reference passes to `{name}_init` (dylib.rs:79-83).
 * level: 1=error 2=warn 3=info 4=debug. May be NULL. */
typedef void (*smhv_log_fn)(int level, const char *msg);

/* reference debug::DebugView (vision-common/src/debug.rs:31-40) */
enum { SMHV_VIEW_NONE = 0, SMHV_VIEW_OCR_INPUT = 1, SMHV_VIEW_FIND_SCALES_INPUT = 2, SMHV_VIEW_LSD_PREPROCESS = 3,
       SMHV_VIEW_LSD_INPUT = 4, SMHV_VIEW_CROPPED_BRQ = 5 };

/* ---- lifecycle ------------------------------------------------------------------------------ */
/* replaces smh_vision_gpu_init (dylib.rs:77-88 -> CudaInstance::init, vision-gpu/src/cuda.rs:31-94) */
SMHV_API int smhv_init(int device, smhv_log_fn log, smhv_ctx **out);
/* replaces smh_vision_gpu_shutdown (dylib.rs:90-97); idempotent, NULL-safe */
SMHV_API void smhv_shutdown(smhv_ctx *ctx);
/* replaces Vision::thread_ctx (vision-gpu/src/lib.rs:154-165): binds the device to the calling thread */
SMHV_API int smhv_thread_ctx(smhv_ctx *ctx);
/* The 3600 ray directions of find_longest_line are `((i as f32) / 10.0).to_radians()` through the PLATFORM libm's
 * cosf / sinf (vision-cpu/src/lib.rs:398-399), so the reference itself is not bit-stable across platforms.  The library
 * ships the glibc 2.35 values (csrc/ray_table.inc): line end points are bit-exact against a Linux/glibc build of
 * vision-cpu.  A host on another libm (Windows UCRT, musl, ...) passes its own f32::cos / f32::sin values here once
 * after smhv_init to get the same guarantee against its own build.  dx, dy: 3600 floats each.  The table is per DEVICE: the
 * call synchronises the device and rebuilds the derived offset tables of every open context on it; no other thread may be
 * launching line searches on that device while it runs. */
SMHV_API int smhv_set_ray_table(smhv_ctx *ctx, const float *dx, const float *dy);
/* thread-local message of the last failing call on this thread ("" if none) */
SMHV_API const char *smhv_last_error(void);

/* ---- screen-relative bounds (vision-common/src/screen.rs:4-66, consts/mod.rs:7-19) ----------- */
/* MAP_BOUNDS.into_absolute + "map fills remaining space" (vision-cpu/src/lib.rs:137-145) */
SMHV_API int smhv_map_bounds(uint32_t frame_w, uint32_t frame_h, uint32_t xywh[4]);
/* CLOSE_DEPLOYMENT_BUTTON_BOUNDS.into_absolute */
SMHV_API int smhv_button_bounds(uint32_t frame_w, uint32_t frame_h, uint32_t xywh[4]);

/* ---- per-frame trait surface ---------------------------------------------------------------- */
/* Vision::load_frame (vision-gpu/src/lib.rs:167-193).  bgra: tightly packed BGRA8, w*h*4 bytes, host
 * memory.  The bytes are copied; the caller keeps ownership (the Rust shim keeps the Arc<VisionFrame>
 * for get_cpu_frame itself).  (Re)allocates device buffers when the dimensions change. */
SMHV_API int smhv_load_frame(smhv_ctx *ctx, const uint8_t *bgra, uint32_t w, uint32_t h);
/* The sub-view case of load_frame (vision-gpu/src/lib.rs:175-179): the frame is the w x h rectangle at (x, y) of a
 * tightly packed parent_w x parent_h BGRA8 image (VisionFrame = OwnedSubImage, util/src/image.rs:238-262). */
SMHV_API int smhv_load_frame_view(smhv_ctx *ctx, const uint8_t *parent_bgra, uint32_t parent_w, uint32_t parent_h,
                                  uint32_t x, uint32_t y, uint32_t w, uint32_t h);
/* Same, but the frame already lives in device memory (zero-copy path for device-side producers). */
SMHV_API int smhv_load_frame_device(smhv_ctx *ctx, const void *d_bgra, uint32_t w, uint32_t h);

/* Vision::crop_to_map (vision-cpu/src/lib.rs:110-171).  *map_open = 0 reproduces Ok(None) (red button
 * fraction < 0.65): nothing else is written.  Otherwise roi = [x,y,w,h] and, if ui_rgba != NULL,
 * w*h*4 bytes of RGBA (grayscale: luma,luma,luma,255) are written to it. */
SMHV_API int smhv_crop_to_map(smhv_ctx *ctx, int grayscale, int *map_open, uint32_t roi[4], uint8_t *ui_rgba);
/* ... and the form that does not wait for the image: with ui_rgba == NULL crop_to_map returns as soon as the button test is known
 * (one host wait; the pass over the ROI, the marker mask and the minimap walk are enqueued with it), and the ui_map travels to
 * pinned host memory of the context on a stream of its own while the caller starts its two branches -- what the reference's
 * PinnedGpuImage is to its GPU back-end (vision-gpu/src/gpuimage.rs:117-166: copied when somebody looks).  smhv_ui_map waits for
 * that copy and hands out the pinned image: w x h RGBA8, tightly packed, readable until the SECOND crop_to_map after this
 * frame's (two buffers take turns).  SMHV_E_STATE when the map is closed. */
SMHV_API int smhv_ui_map(smhv_ctx *ctx, const uint8_t **rgba, uint32_t *w, uint32_t *h);
/* number of "Close Deployment" red pixels counted by the last crop_to_map (diagnostic) */
SMHV_API int smhv_red_pixels(smhv_ctx *ctx, uint32_t *count);

/* Vision::ocr_preprocess (vision-cpu/src/lib.rs:173-231): *out is a borrowed host pointer to
 * (w/2)*(h/2) bytes, valid until the next ocr_preprocess / load_frame on this context. */
SMHV_API int smhv_ocr_preprocess(smhv_ctx *ctx, const uint8_t **out, size_t *len);
/* Vision::find_scales_preprocess (vision-cpu/src/lib.rs:233-251): borrowed host image; rows above
 * scales_start_y keep whatever the previous call left there (as in the reference). */
SMHV_API int smhv_find_scales_preprocess(smhv_ctx *ctx, uint32_t scales_start_y, const uint8_t **out, uint32_t *w, uint32_t *h);

/* Vision::isolate_map_markers (vision-cpu/src/lib.rs:253-280) */
SMHV_API int smhv_isolate_map_markers(smhv_ctx *ctx);
/* Vision::mask_marker_lines (vision-cpu/src/lib.rs:357-375): threshold + L1 radius-1 dilation */
SMHV_API int smhv_mask_marker_lines(smhv_ctx *ctx);
/* Host copy of the LSD mask (w*h bytes, values {0,255}) == "detected marker pixel coords". */
SMHV_API int smhv_get_lsd_image(smhv_ctx *ctx, uint8_t *out, uint32_t *w, uint32_t *h);
/* Vision::find_longest_line (vision-cpu/src/lib.rs:387-449) on the context's LSD image */
SMHV_API int smhv_find_longest_line(smhv_ctx *ctx, float px, float py, float max_gap, smhv_line *line, float *len_sq);
/* Vision::find_marker_lines (vision-cpu/src/lib.rs:377-385 -> lsd::find_lines::<32>, lsd.rs:60-107) */
SMHV_API int smhv_find_marker_lines(smhv_ctx *ctx, uint32_t max_gap, smhv_line out[SMHV_MAX_LINES], uint32_t *n);
/* rounds (find_longest_line invocations) and mask samples of the last smhv_find_marker_lines; exact != 0 repeats the
 * scan with every ray cast (sample count == the reference's).  Diagnostic. */
SMHV_API int smhv_lsd_stats(smhv_ctx *ctx, uint32_t max_gap, int exact, uint32_t *rounds, uint64_t *ray_steps);
/* calc_meters_to_px_ratio (src/vision/mpx_ratio.rs:3-134) on the image of the last
 * find_scales_preprocess.  scales = n x {meters, x, y} (OCR label anchors, BRQ coordinates), n <= 3.
 * *has = 0 reproduces None.  bars (optional) = n x {left, y, right, found} (the scales_debug lines). */
SMHV_API int smhv_calc_meters_to_px_ratio(smhv_ctx *ctx, const uint32_t *scales, uint32_t n, double *ratio, int *has, uint32_t *bars);
/* find_minimap (src/vision/find_minimap.rs:47-146; host code in the reference, run on get_cpu_frame().view(roi)
 * right after crop_to_map, src/vision/mod.rs:85) on the resident frame: four directed walks from the ROI centre
 * over the "edginess" (max neighbour colour distance) of the BGRA frame.  rect = {left, right, top, bottom} in
 * ROI coordinates; *found = 0 reproduces None. */
SMHV_API int smhv_find_minimap(smhv_ctx *ctx, uint32_t rect[4], int *found);
/* Vision::get_debug_view (vision-cpu/src/lib.rs:451-460): RGBA copy; rgba may be NULL to query w,h. */
SMHV_API int smhv_get_debug_view(smhv_ctx *ctx, int which, uint8_t *rgba, uint32_t *w, uint32_t *h);
/* The per-call path's counterpart of the reference's Timeshares waterfall (vision-common/src/debug.rs:3-30; src/vision/mod.rs:54-66
 * wraps every trait call in one): host wall time of every call of the trait surface on this context, summed, and the number of
 * calls, since the context was created or last reset.  The two branches run on two threads: the time of a frame is
 * load_frame + crop_to_map + find_minimap + max(markers branch, scales branch), not the sum of everything. */
#define SMHV_T_LOAD_FRAME 0
#define SMHV_T_CROP_TO_MAP 1
#define SMHV_T_FIND_MINIMAP 2
#define SMHV_T_ISOLATE_MAP_MARKERS 3
#define SMHV_T_MASK_MARKER_LINES 4
#define SMHV_T_FIND_MARKER_LINES 5
#define SMHV_T_OCR_PREPROCESS 6
#define SMHV_T_FIND_SCALES_PREPROCESS 7
#define SMHV_T_CALC_METERS_TO_PX_RATIO 8
#define SMHV_T_GET_DEBUG_VIEW 9
#define SMHV_T_FIND_LONGEST_LINE 10
#define SMHV_T_UI_MAP 11
#define SMHV_TRAIT_CALLS 12
SMHV_API int smhv_trait_times(smhv_ctx *ctx, uint64_t ns[SMHV_TRAIT_CALLS], uint64_t calls[SMHV_TRAIT_CALLS], int reset);

/* ---- batched pipeline (BASELINE configs 2-5): frames resident in HBM -------------------------- */
#define SMHV_STAGE_MARKERS 0x1u /* button test + marker mask + dilation + LSD                  */
#define SMHV_STAGE_UI_MAP 0x2u  /* ui_map RGBA                                                   */
#define SMHV_STAGE_OCR 0x4u     /* ocr_preprocess                                                */
#define SMHV_STAGE_SCALES 0x8u  /* find_scales_preprocess + calc_meters_to_px_ratio (needs anchors) */
#define SMHV_STAGE_ALL 0xFu
#define SMHV_STAGE_MINIMAP 0x10u /* find_minimap (not a Vision trait method; the caller's next step, not in STAGE_ALL) */
#define SMHV_STAGE_EXACT_STATS 0x20u /* diagnostic: cast every ray of every visited pixel, so that `ray_steps` equals the
                                        reference's sample count.  Without it the LSD skips angular sectors that provably
                                        cannot hold an acceptable ray -- a sector is cast only if it sees a white pixel
                                        50 - T .. 50 steps away, T = max_gap: a ray without one is aborted before it is long
                                        enough; a library built with -DSMH_CULL_CHAIN also asks for one 50 - 2T - 1 ..
                                        50 - T - 1 steps away, by the same argument (lines, rounds and every other output
                                        are identical; ray_steps then counts only the samples actually taken, by the
                                        sectors that were not skipped). */

#define SMHV_STAGE_LSD_HELPERS 0x40u /* tuning (smhv_batch_run; a depth-1 pipeline sets it itself): workgroups of k_lsd that have finished their own frame help
                                       the frames still being searched (ray-cast candidates ahead of the owner; results are
                                       identical either way).  Shortens a single batch with a few heavy frames; only gets in
                                       the way when several batches are pipelined, so it is off by default. */

/* One record per frame (what a node-level gather moves between GPUs).  mpx/derived fields follow
 * src/ui/mod.rs:131-140 (length_px, meters in f64) and src/ui/markers.rs:98 (angle = atan2f). */
typedef struct {
	uint32_t map_open;              /* 0 = Ok(None): every other field is 0                        */
	uint32_t n_lines;
	smhv_line lines[SMHV_MAX_LINES];
	double mpx;                     /* meters per pixel, valid iff has_mpx                         */
	uint32_t has_mpx;
	uint32_t n_mask_px;             /* 255-pixels in the dilated marker mask                       */
	uint32_t red_pixels;            /* close-deployment button count                               */
	uint32_t rounds;                /* find_longest_line invocations (workload statistic)          */
	uint64_t ray_steps;             /* mask samples taken by the rays that were cast (== the reference's count
	                                   when SMHV_STAGE_EXACT_STATS is set)                          */
	double length_px[SMHV_MAX_LINES];
	double meters[SMHV_MAX_LINES];  /* length_px * mpx (0 when !has_mpx)                           */
	float angle[SMHV_MAX_LINES];
	uint32_t minimap[4];            /* find_minimap: {left, right, top, bottom} in map-ROI coordinates  */
	uint32_t has_minimap;           /* 1 iff SMHV_STAGE_MINIMAP ran and the map is open                 */
	uint32_t status;                /* SMHV_FRAME_OK, or why this frame has no valid marker lines (SMHV_FRAME_*) */
} smhv_frame_result;

/* smhv_frame_result.status.  The reference logs and drops a frame on any Err of a trait method
 * (src/vision/mod.rs:272-276); a frame whose status is not SMHV_FRAME_OK is to be dropped the same way.
 *   SMHV_FRAME_LSD_STUCK: the line search's watchdog gave the frame up (its waves made no progress for the spin budget --
 *   never observed outside the test that lowers the budget).  The record then has n_lines = 0 and rounds = 0xFFFFFFFF; every
 *   other stage output of the frame (ui_map, mask, ocr, scales, m/px) is valid.  smhv_batch_read_results,
 *   smhv_pipeline_wait(_all) and smhv_node_gather return SMHV_E_STATE when a frame of the run they cover has a non-zero
 *   status (the message names the first such frame and carries the watchdog's state dump); the records are still copied
 *   out, so the caller can drop exactly the frames whose status is set.  The condition is reported once, by the first
 *   of those calls that sees it. */
#define SMHV_FRAME_OK 0u
#define SMHV_FRAME_LSD_STUCK 1u

/* per-frame OCR anchors for SMHV_STAGE_SCALES: OCR (Tesseract) is outside this library; where the labels are, the bars under them and the
 * glyph crops to read: "scale labels" below (smhv_scale_labels_anchors makes these anchors from the numbers read) */
typedef struct {
	uint32_t n;                     /* 0..3                                                        */
	uint32_t scales_start_y;        /* min(ocr.bottom), src/vision/mod.rs:182                      */
	uint32_t scales[SMHV_MAX_SCALES][3]; /* {meters, x, y}                                         */
} smhv_anchors;

typedef struct {
	uint32_t frame_w, frame_h;
	uint32_t roi[4], button[4];     /* map / button rects in frame coordinates                     */
	uint32_t brq_w, brq_h;
	/* device output layouts: row pitches in bytes, per-frame strides in bytes, and the byte offset
	 * of pixel (0,0) inside a frame's slab (rows are padded so 16-byte stores stay aligned)        */
	uint64_t ui_pitch, ui_stride, ui_offset;         /* RGBA8                                       */
	uint64_t mask_pitch, mask_stride, mask_offset;   /* u8 {0,255}                                  */
	uint64_t ocr_pitch, ocr_stride, ocr_offset;      /* u8                                          */
	uint64_t scales_pitch, scales_stride, scales_offset; /* u8 {0,255}                              */
	uint64_t bits_pitch_words, bits_stride, bits_xoff;   /* bit-packed mask: bit (x+xoff) of row y */
} smhv_batch_layout;

SMHV_API int smhv_batch_create(smhv_ctx *ctx, uint32_t frame_w, uint32_t frame_h, uint32_t max_frames, smhv_batch **out);
SMHV_API void smhv_batch_destroy(smhv_batch *b);
SMHV_API int smhv_batch_layout_get(smhv_batch *b, smhv_batch_layout *out);
/* Runs the selected stages over n resident frames (d_frames: n * frame_w*frame_h*4 bytes of BGRA8 in
 * device memory) on `stream` (a hipStream_t, NULL = default stream).  Asynchronous and non-blocking: every kernel and
 * copy is enqueued on `stream` and the call returns; results are in device memory when the stream reaches this point.
 * anchors: host array of n smhv_anchors or NULL (copied into pinned staging before the call returns).
 * Alignment of d_frames (here and in smhv_pipeline_submit / smhv_node_run): a pixel, 4 bytes -- nothing more.  Frames are tightly
 * packed, so with a width that is no multiple of 4 every row, and every frame after the first, starts 4, 8 or 12 bytes off a
 * 16-byte boundary anyway; the kernels' 16-byte loads take any 4-byte aligned address and a base pointer at such an offset gives
 * the same outputs, bit for bit (16-byte alignment and frame_w % 4 == 0 are merely the fastest case).  A pointer that is not
 * 4-byte aligned is refused with SMHV_E_INVALID before anything is enqueued.
 * Indices >= n (here and in smhv_pipeline_submit, for the slot's batch): a run over n < max_frames frames touches nothing of the
 * frames from n on -- every kernel of the run is launched over n frames.  Their records, images, bit rows and tile-major masks stay,
 * byte for byte, what the newest earlier run of this batch that covered the index left (zeroes where none did), and the slabs the
 * library makes on demand (d_mask, d_ui) are brought up to date for every frame any run since the last read covered, not only for
 * this run's n.  Within 0 .. n - 1 a frame the run finds closed gets its record and keeps its older images and bit rows; its
 * tile-major mask then reads as not written (smhv_batch_read_tile_mask). */
SMHV_API int smhv_batch_run(smhv_batch *b, const void *d_frames, uint32_t n, uint32_t stages, int grayscale, uint32_t max_gap,
                            const smhv_anchors *anchors, void *stream);
/* device pointers of the batch outputs (valid for the life of the batch); any of them may be NULL.
 * d_mask, the marker mask one byte per pixel, is the one slab the runs do not write by themselves: it is an exact function of the
 * bit-packed rows (byte x of a row = 0xFF where bit x + bits_xoff is set), nothing on the device reads it, and the library makes it
 * from the bit rows when one of ITS readers wants it (smhv_batch_read_image, smhv_batch_render_layers / smhv_batch_feed_view with the
 * mask as the map).  A call with a non-NULL d_mask tells the library that the caller reads the slab itself: the call waits for the
 * device, brings the bytes of every run so far up to date, and switches the batch for good -- every later run (smhv_batch_run, or a
 * pipeline's submission into this batch) writes its frames' bytes with one more small kernel on its own stream right behind its
 * streaming pass (in a frame-granular pipeline ahead of the publication, so inside the submission's completion).  So the rule for
 * every pointer here stays "a run's results are in memory when its stream gets there"; a caller that never asks for d_mask never
 * pays for it (19 % of the streaming pass's written bytes at 1080p).
 * d_ui, the ui_map as RGBA8, is owed in the same way by GREY runs: a grey ui_map is (l, l, l, 255), so a grey run (grayscale != 0,
 * without SMHV_STAGE_HEIGHTMAP_OVERLAY) writes one luma byte per pixel into a plane of the library's own, and the library makes the
 * RGBA rows from it when one of ITS readers wants them (smhv_batch_read_image, smhv_batch_render*, smhv_batch_probe /
 * smhv_batch_render_debug, smhv_batch_feed*), on the stream that call is given.  Colour runs and overlay runs write d_ui directly,
 * and a frame a run finds closed keeps its older image whichever run wrote it.  A call with a non-NULL d_ui is the same switch as
 * for d_mask: it waits for the device, brings the slab up to date, and from then on grey runs of this batch write RGBA themselves.
 * Pass NULL for d_ui unless you read the slab with a kernel or a copy of your own: two thirds of the grey streaming pass's written
 * bytes at 1080p are the three bytes per pixel it saves. */
SMHV_API int smhv_batch_device_ptrs(smhv_batch *b, void **d_results, void **d_ui, void **d_mask, void **d_ocr, void **d_scales, void **d_bits);
/* The marker mask a third time, as the streaming passes leave it for the line search (and for any host kernel that wants the
 * marker pixels without scanning a 1-4 % full image): TILE-MAJOR, 32 x 8 px tiles of the bit-packed rows -- tile (ty, wx) = rows
 * 8 ty .. 8 ty + 7 of word column wx (bits_pitch_words word columns, bit (x + bits_xoff) of a row = pixel x), eight consecutive
 * 32-bit words at d_tiled[frame * tile_rows * word_columns * 8 + (ty * word_columns + wx) * 8] -- written ONLY for tiles that hold a
 * set bit, and one occupancy byte per (tile row, group of eight word columns) saying which: bit j of
 * d_occ[frame * tile_rows * occ_pitch + ty * occ_pitch + g] = tile (ty, 8 g + j) is non-empty (every byte of an open frame's tile rows
 * is written).  Rows of the last tile row beyond the image are undefined.  A run writes them when its bands are whole tile rows --
 * the library takes such bands where they cost the streaming pass nothing or pay (ROIs up to 900 rows, i.e. frames up to 1080p, and
 * every size whose band count does not grow by it); smhv_batch_read_tile_mask reports per frame whether the last run did.
 * geometry[4] <- {tile_rows, word_columns, occ_pitch, bits_xoff}. */
SMHV_API int smhv_batch_tile_mask(smhv_batch *b, void **d_tiled, void **d_occ, uint32_t geometry[4]);
/* synchronising host copies of one frame's tile-major mask, occupancy bytes and bit-packed rows (any of them may be NULL);
 * *written <- 1 when the last run over that frame wrote the tile-major mask and the occupancy bytes, 0 when it wrote the bit rows only */
SMHV_API int smhv_batch_read_tile_mask(smhv_batch *b, uint32_t frame, uint32_t *tiled, uint8_t *occ, uint32_t *bits, int *written);
/* synchronising host copies (tightly packed) */
SMHV_API int smhv_batch_read_results(smhv_batch *b, uint32_t first, uint32_t n, smhv_frame_result *out);
SMHV_API int smhv_batch_read_image(smhv_batch *b, int which /* SMHV_VIEW_* or 100 = ui_map RGBA */, uint32_t frame, uint8_t *out);
/* Per-stage device time, AVERAGED over the timed smhv_batch_run calls since the last read (at most the
 * 64 most recent), measured with hipEvents on
 * the run's stream (the analogue of the reference's Timeshares, vision-common/src/debug.rs:3-30).
 * ms[0]=button ms[1]=map pass ms[2]=brq pass ms[3]=lsd ms[4]=scale ratio.  Synchronises. */
/* Kept for source compatibility; has no effect: the batched pipeline runs entirely on the stream given to
 * smhv_batch_run (the quadrant stages are fused into the streaming pass, the scale scan into the record kernel). */
SMHV_API int smhv_batch_set_scales_stream(smhv_batch *b, void *stream);
/* Make `stream` wait until the streaming pass (k_map_pass) of b's most recent smhv_batch_run has finished.  (What
 * smhv_pipeline_submit uses to start pipelined batches half a period apart; a host that pipelines smhv_batch objects by
 * hand can do the same.) */
SMHV_API int smhv_batch_wait_map_pass(smhv_batch *b, void *stream);
SMHV_API int smhv_batch_enable_timing(smhv_batch *b, int enable);
/* diagnostic: per-frame cooperation counters of the most recent line-segment launch, 4 words per frame:
 * {groups of the owner that had helpers attached, candidates it took from the helpers' cache, candidates cast by helpers,
 *  requests posted}.  Synchronises. */
SMHV_API int smhv_batch_lsd_coop_stats(smhv_batch *b, uint32_t first, uint32_t n, uint32_t *out);
SMHV_API int smhv_batch_stage_ms(smhv_batch *b, float ms[5]);

/* ---- pipeline: several batches in flight, scheduled by the library ----------------------------------------------
 * `depth` output buffer sets (smhv_batch objects) of max_frames frames.  The library owns every stream of the schedule (created
 * in a fixed order: the throughput does not depend on what streams the host created before or on how it interleaves its calls).
 *   submit : asynchronous.  Enqueues the stages for n resident frames on the next slot (round robin) and returns at
 *            once; it only waits when that slot's previous submission (`depth` submissions ago) is still running.
 *            after_stream (optional): a stream whose already enqueued work (e.g. the producer of d_frames) must finish
 *            first.  *slot receives the slot index.
 *   wait   : host waits for the slot's most recent submission (all of its frames' records are in device memory then).
 *   slot   : the slot's batch object (results, device pointers, images); with `stream` != NULL also a stream a consumer can use
 *            -- with the frame-granular search the call first WAITS (host) for the slot's submission: a submission's completion
 *            is a counter the search's waves count down, not a point on a stream.
 *   hold   : a consumer reads the slot's outputs on `stream` (work already enqueued there): the slot's next submission
 *            is ordered behind it.
 * depth: 1..32.  Two line-search schedules (smhv_pipeline_options::search pins one):
 *   batch-granular: one search launch per submission on the slot's own stream (k_lsd with helper workgroups at depth 1, k_lsd
 *     at depth 2 up to 1080p, k_lsd_tile -- eight waves per frame -- otherwise), staggered starts, and from depth 3 on an
 *     occupancy policy for the streaming pass and late helpers for heavy frames, both adapting to the workload.  Every slot's
 *     stream has a hardware queue of its own (up to 16 per pipeline, 20 for all live pipelines of the process on one device).
 *   frame-granular (depth >= 3, frame sizes up to ~4K): ONE long-lived search kernel per pipeline whose waves pull (slot,
 *     frame) items from a device-side ring -- one wave per frame, the reference's sequential scan, with the other waves of its
 *     workgroup casting a heavy frame's upcoming candidates -- write the frame's record and count it off against its
 *     submission; the submissions' streaming sides take two library-owned streams in turn.  A slot is done when its slowest
 *     frame is, nothing else waits for that frame.  The kernel closes by itself when nothing is outstanding (a device-wide
 *     synchronize by anybody still returns) and is launched again by the next submission.  A third of the wave-time per frame,
 *     but a frame is one wave's work from start to end: it needs ~3000 light frames in flight (three per resident wave: 12 x
 *     256 frames at 1080p, 526-538 k frames/s; more changes nothing).
 *     A frame that is still at work when most of its submission is done asks idle waves of OTHER workgroups as well (they copy its
 *     mask tiles from global memory and answer through a ring of 8/16-byte granules; smhv_pipeline_options::remote_*).
 *   SMHV_SEARCH_AUTO (the default): below depth 6 batch-granular.  From depth 6 on the pipeline has both and MEASURES which is
 *     faster on the workload it is given -- a window of 8 x depth submissions in each, after warm-ups, ~24 x depth submissions in
 *     all; again every 16384 submissions and when the submissions change shape for good (frames per submission by more than 25 %,
 *     stages or gap threshold, for `depth` submissions in a row; at most four such re-measurements between two periodic ones) --
 *     keeping the faster one (both write byte-identical records).  Measured at depth 12: the synthetic 256 x 1080p scene 540 k
 *     frames/s on the frame-granular search (430 k batch-granular); the reference's own 1440p screenshots in batches of 128 (0-372
 *     search rounds per frame) 300 k batch-granular, 243 k frame-granular (210 k without the help across workgroups); at depth 20
 *     (24 GB of output slots) 290-300 k on either.
 *   Completion: only smhv_pipeline_wait / smhv_pipeline_wait_all / smhv_pipeline_slot(.., &stream) guarantee a submission's
 *     records.  A frame-granular submission's completion is not a point on any stream: a device-wide synchronize returns when the
 *     search kernel has closed, which it also does after 20 ms without progress (e.g. behind a slow producer on `after_stream`) --
 *     the library's waits launch it again, a bare hipDeviceSynchronize does not.
 *   smhv_debug_skip_line_search and stage_ms[3..4] of smhv_batch_stage_ms apply to batch-granular submissions only (a frame-granular
 *     submission's search and records are the service's: smhv_debug_pipeline_stats; both in smh_vision_hip_debug.h). */
typedef struct smhv_pipeline smhv_pipeline;
SMHV_API int smhv_pipeline_create(smhv_ctx *ctx, uint32_t frame_w, uint32_t frame_h, uint32_t max_frames, uint32_t depth, smhv_pipeline **out);
/* The same with explicit choices: zero-initialise, set `size` = sizeof(smhv_pipeline_options), change what you need (every 0 is
 * the library's default; there are no environment variables). */
#define SMHV_SEARCH_AUTO 0u             /* batch-granular below depth 6; from 6 on whichever of the two the pipeline measures faster on its workload */
#define SMHV_SEARCH_BATCH 1u
#define SMHV_SEARCH_FRAME 2u            /* SMHV_E_INVALID when depth < 3 or the frame's mask tiles do not fit the LDS beside the streaming pass (8K) */
#define SMHV_PIPE_NO_TEAM_HELP 1u       /* flags, diagnostics (A/B): frame-granular search without waves helping the heavy frames of their workgroup */
#define SMHV_PIPE_NO_STREAM_PRIORITY 2u /*   ... without wave priority for the streaming pass */
#define SMHV_PIPE_NO_PROLOGUE 4u        /*   ... button test and anchor upload on the streaming streams instead of a stream of their own */
#define SMHV_PIPE_NO_REMOTE_HELP 8u     /*   ... a heavy frame is helped by the waves of its own workgroup only, not by idle waves of other workgroups */
#define SMHV_PIPE_WALK_BIT_ROWS 32u     /*   ... the service builds a frame's tile store by walking the bit rows' bounding box (rounds 2-5) instead of from the pass's tile-major mask */
#define SMHV_PIPE_THREE_LOAD_SETS 64u   /*   ... the streaming pass of a frame-granular pipeline with three register sets of loads in flight (128 registers: two workgroups per CU beside the service; round 5's form up to 1080p) instead of two (112: three) */
#define SMHV_PIPE_HELP_FIRST 16u        /*   ... frames ask other workgroups, and waves answer, even while frames are waiting for a wave (default: only then not) */
typedef struct {
	uint32_t size;
	uint32_t search;                    /* SMHV_SEARCH_* */
	uint32_t streams;                   /* frame-granular: streaming streams the submissions take in turn (0 = 2; 1..8) */
	uint32_t idle_close_us;             /* frame-granular: the search kernel closes after this long without work when nothing is outstanding (0 = 45) */
	uint32_t occupancy_policy;          /* batch-granular, depth >= 3: 0 = adaptive (on unless the workload is search-bound), 1 = always on, 2 = off */
	uint32_t late_helpers;              /* batch-granular: workgroups that have finished their frame help one still at work: 0 = when the
	                                       workload is search-bound, 1 = always, 2 = never */
	uint32_t service_workgroups;        /* frame-granular, diagnostic: workgroups of the search kernel (0 = one per CU) */
	uint32_t flags;                     /* SMHV_PIPE_* */
	uint32_t remote_after;              /* frame-granular: search rounds after which a frame asks the waves of OTHER workgroups for help (0 = 24) */
	uint32_t remote_tickets;            /*   ... and how many of them it asks for (0 = 3; at most 12 attach) */
	uint32_t remote_last;               /*   ... once at most 1 / remote_last of its submission's frames are still at work (0 = 6) */
	uint32_t room_for_others;           /* frame-granular: 1 = the search kernel leaves an eighth of the CUs without a workgroup of its own, so that kernels of
	                                       OTHER owners (RCCL's: 21 KB of LDS and 280 VGPRs per workgroup; torch's) always find a CU to run on beside the pipeline.
	                                       A search workgroup holds most of its CU's LDS for as long as the pipeline is busy: with one on EVERY CU (the default
	                                       up to 1080p: the fastest when the pipeline has the GPU to itself, +7 %) such a kernel waits until the pipeline runs
	                                       dry -- and holds up the queues behind it meanwhile (measured: seconds, and a quarter of the pipeline's rate).
	                                       smhv_node_create sets it (its gather is an RCCL kernel); set it when the process launches anything else beside a
	                                       pipeline.  0 = the library's choice (off; on for smhv_node), 1 = on, 2 = off */
} smhv_pipeline_options;
SMHV_API int smhv_pipeline_create_ex(smhv_ctx *ctx, uint32_t frame_w, uint32_t frame_h, uint32_t max_frames, uint32_t depth,
                                     const smhv_pipeline_options *options, smhv_pipeline **out);
SMHV_API void smhv_pipeline_destroy(smhv_pipeline *p);
/* n may differ from submission to submission (1 .. max_frames): what the slot holds at indices >= n is what its earlier submissions
 * left there -- the rule at smhv_batch_run. */
SMHV_API int smhv_pipeline_submit(smhv_pipeline *p, const void *d_frames, uint32_t n, uint32_t stages, int grayscale, uint32_t max_gap,
                                  const smhv_anchors *anchors, void *after_stream, uint32_t *slot);
SMHV_API int smhv_pipeline_wait(smhv_pipeline *p, uint32_t slot);
SMHV_API int smhv_pipeline_wait_all(smhv_pipeline *p);
SMHV_API int smhv_pipeline_slot(smhv_pipeline *p, uint32_t slot, smhv_batch **batch, void **stream);
SMHV_API int smhv_pipeline_hold(smhv_pipeline *p, uint32_t slot, void *stream);

/* ---- node: every GPU of a machine from ONE process -------------------------------------------
 * Frames are independent: a global batch is block-sharded over the devices (smhv_shard_range), each device runs the
 * single-GPU pipeline on its resident shard, and the only exchange is one ncclGather (RCCL over xGMI, rccl.h:745) of the
 * per-frame result records to devices[0].  RCCL is dlopen'ed by smhv_node_create (SMHV_E_NO_DEVICE if it is absent).
 *   run    : asynchronous; d_frames[i] = n[i] resident frames on devices[i] (n[i] <= max_frames_per_device, may be 0),
 *            anchors[i] (optional) the shard's anchors.
 *   gather : all records of the most recent run in device order (sum of n[i]) into `out`; synchronises.
 *   ctx    : the per-device context / pipeline (for uploads, images, device pointers).
 *   depth  : slots of every device's pipeline; 0 = 12 (what bench.py runs one GPU with).  The pipelines are created with
 *            smhv_pipeline_options::room_for_others: the gather's RCCL kernel has to find a CU beside the search kernel. */
typedef struct smhv_node smhv_node;
SMHV_API void smhv_shard_range(uint64_t n_total, uint32_t rank, uint32_t world, uint64_t *lo, uint64_t *hi);
SMHV_API int smhv_node_create(const int *devices, uint32_t n_devices, uint32_t frame_w, uint32_t frame_h, uint32_t max_frames_per_device,
                              uint32_t depth, smhv_log_fn log, smhv_node **out);
SMHV_API void smhv_node_destroy(smhv_node *node);
SMHV_API int smhv_node_ctx(smhv_node *node, uint32_t i, smhv_ctx **ctx, smhv_pipeline **pipe);
SMHV_API int smhv_node_run(smhv_node *node, const void *const *d_frames, const uint32_t *n, uint32_t stages, int grayscale, uint32_t max_gap,
                           const smhv_anchors *const *anchors);
SMHV_API int smhv_node_gather(smhv_node *node, smhv_frame_result *out, uint32_t *n_total);

/* ---- ingest queue: the capture hand-off in front of load_frame (src/capture.rs:33-63) --------------------------
 * The reference's capture thread hashes each captured BGRA frame with crc32fast::hash (CRC-32/IEEE) and passes it
 * on only if the CRC differs from the previous capture's (capture.rs:44-47, `last_frame_crc32` starts at 0).  Here
 * the capture source fills pinned staging buffers (acquire -> write -> commit), every frame goes to HBM with an
 * asynchronous copy on the queue's own stream, its CRC-32 is computed on the device, and frames that are not
 * duplicates of the last accepted frame are appended, in order, to a device slab of `capacity` frames that
 * smhv_batch_run (or smhv_load_frame_device) consumes.  One producer thread per queue. */
typedef struct smhv_ingest smhv_ingest;
SMHV_API int smhv_ingest_create(smhv_ctx *ctx, uint32_t frame_w, uint32_t frame_h, uint32_t slots, uint32_t capacity, smhv_ingest **out);
/* The same with flags.  SMHV_INGEST_ROI_UPLOAD: the CRC-32 of every committed frame is computed on the HOST (worker threads of the
 * queue, carry-less-multiply folding: the whole frame, as the reference hashes it) and only what the pipeline reads -- the map
 * ROI's rows and the button's rows, 39 % of a 1080p frame -- travels over PCIe, and nothing at all for a duplicate.  The slab
 * frames then hold exactly those two rectangles (zero elsewhere), which is all smhv_batch_run / the pipelines read.  BGRA8,
 * NV12 and I420 commits only (for the two video layouts see SMHV_PIXELS_NV12 below: the CRC is of the committed YUV bytes). */
#define SMHV_INGEST_ROI_UPLOAD 1u
#define SMHV_INGEST_WORKERS(n) (((n) & 0xFFu) << 8)   /* diagnostic, with SMHV_INGEST_ROI_UPLOAD: hashing threads (0 = the library's choice: one per staging slot, at most half the cores the process may use -- the cgroup CPU quota counts -- and at least two) */
#define SMHV_INGEST_NO_AFFINITY 2u   /* the hashing threads are left to the scheduler (default: on a multi-socket host they run on the CPUs next to the GPU) */
SMHV_API int smhv_ingest_create_ex(smhv_ctx *ctx, uint32_t frame_w, uint32_t frame_h, uint32_t slots, uint32_t capacity, uint32_t flags, smhv_ingest **out);
SMHV_API void smhv_ingest_destroy(smhv_ingest *q);
/* The CPUs next to the queue's GPU (the NUMA node of its PCI device, from sysfs) as a Linux cpulist, e.g. "64-127,192-255"; "" on a
   single-node host or where sysfs does not say.  The queue's hashing threads run there.  The staging buffers are pinned next to
   the GPU, so the thread that FILLS them (the capture thread: `src/capture.rs`) does well to run there too --
   smhv_ingest_bind_thread binds the calling thread to those of them its affinity mask already allows (SMHV_OK and nothing done when
   the list is empty or fewer than two of its CPUs are allowed; the binding stays until the caller changes it).  The hashing threads
   are bound the same way, and only when the allowed CPUs on the GPU's side are at least as many as the threads.  Measured on a
   two-socket MI355X host, 1080p frames, the queue alone: 11.8 k frames/s from the GPU's socket, 7.3 k from the other, 9.4-11.5 k
   when the scheduler chooses. */
SMHV_API int smhv_ingest_local_cpus(smhv_ingest *q, char *buf, size_t cap);
SMHV_API int smhv_ingest_bind_thread(smhv_ingest *q);
/* next pinned staging buffer (frame_w * frame_h * 4 bytes); blocks only when all `slots` uploads are in flight */
SMHV_API int smhv_ingest_acquire(smhv_ingest *q, uint8_t **host_bgra);
/* start upload + CRC of the acquired buffer; returns at once */
SMHV_API int smhv_ingest_commit(smhv_ingest *q);
/* acquire + memcpy + commit for frames that live in ordinary host memory */
SMHV_API int smhv_ingest_push(smhv_ingest *q, const uint8_t *bgra);
/* Frames that come out of an image decoder instead of the screen capture (src/ui/debug.rs:169:
 * `image::load_from_memory(..).into_bgra8()`): the staging buffer holds frame_w * frame_h pixels in the decoder's layout,
 * they are uploaded as they are and converted to BGRA8 on the device exactly as image 0.23's into_bgra8 does for 8-bit
 * images (RGB: alpha = 255; L / LA: b = g = r = l), BEFORE the CRC, so the duplicate rule sees the reference's bytes. */
#define SMHV_PIXELS_BGRA8   0u
#define SMHV_PIXELS_RGBA8   1u
#define SMHV_PIXELS_RGB8    2u
#define SMHV_PIXELS_LUMA8   3u
#define SMHV_PIXELS_LUMA_A8 4u
/* Frames that come out of a VIDEO decoder: 8-bit 4:2:0 planes, 1.5 bytes per pixel.  For a frame of w x h, cw = (w + 1) / 2 and
 * ch = (h + 1) / 2 (odd sizes are legal).  Tight layouts, as the staging buffer holds them:
 *   SMHV_PIXELS_NV12: the Y plane (w x h), then one plane of interleaved U, V pairs (cw pairs x ch rows).
 *   SMHV_PIXELS_I420: Y, then U (cw x ch), then V (cw x ch).
 * The colour description rides in the upper bits of the same word -- SMHV_PIXELS_YUV(layout, matrix, range, chroma):
 *   matrix 0 = BT.709, 1 = BT.601;  range 0 = limited, 1 = full;  chroma 0 = nearest, 1 = bilinear.  Any other bit: SMHV_E_INVALID.
 * The arithmetic, in int32 with >> the arithmetic shift:  c = cy * (Y - yoff), d = U' - 128, e = V' - 128,
 *   R = clip8((c + rv * e + 128) >> 8), G = clip8((c - gu * d - gv * e + 128) >> 8), B = clip8((c + bu * d + 128) >> 8), A = 255,
 * output bytes B, G, R, A, with (the real matrices times 256, rounded: within 1 level of the rounded float64 result everywhere)
 *                    cy  yoff   rv   gu   gv   bu
 *   709 limited     298   16   459   55  136  541
 *   601 limited     298   16   409  100  208  516
 *   709 full        256    0   403   48  120  475
 *   601 full        256    0   359   88  183  454
 * Chroma of pixel (x, y):  nearest: U' = U[y >> 1][x >> 1].  Bilinear, centre-sited: cx = x >> 1, cy_ = y >> 1,
 *   nx = clamp(cx + ((x & 1) ? 1 : -1), 0, cw - 1), ny = clamp(cy_ + ((y & 1) ? 1 : -1), 0, ch - 1),
 *   U' = (9 U[cy_][cx] + 3 U[cy_][nx] + 3 U[ny][cx] + U[ny][nx] + 8) >> 4.  The same for V.
 * In the queue the frame is uploaded as it is (1.5 bytes per pixel) and converted on the device.  A plain queue converts in front
 * of the device CRC, as for the other decoder layouts: its CRC is of the CONVERTED BGRA bytes.  A queue created with
 * SMHV_INGEST_ROI_UPLOAD hashes on the host what was committed: its CRC is of the SOURCE bytes, the whole tight YUV frame
 * (smhv_ingest_staging_bytes of them); it uploads the Y rows of the map ROI and of the button with the chroma rows and columns
 * they need, and converts them into the slab frame.  Both CRCs are functions of the frame, so a repeated capture is a duplicate
 * either way; they are different numbers.  The layout is kept per staging slot: BGRA and YUV commits may alternate. */
#define SMHV_PIXELS_NV12    5u
#define SMHV_PIXELS_I420    6u
#define SMHV_YUV_BT709 0u
#define SMHV_YUV_BT601 1u
#define SMHV_YUV_LIMITED 0u
#define SMHV_YUV_FULL 1u
#define SMHV_YUV_NEAREST 0u
#define SMHV_YUV_BILINEAR 1u
#define SMHV_PIXELS_YUV(layout, matrix, range, chroma) ((uint32_t)(layout) | ((uint32_t)(matrix) << 8) | ((uint32_t)(range) << 9) | ((uint32_t)(chroma) << 10))
SMHV_API int smhv_ingest_commit_pixels(smhv_ingest *q, uint32_t layout);
SMHV_API int smhv_ingest_push_pixels(smhv_ingest *q, const uint8_t *pixels, uint32_t layout);
/* how many bytes of a staging buffer (from its start) a frame of w x h in `pixels` fills; 0 for an unknown layout or a zero size.
   Needs no device. */
SMHV_API uint64_t smhv_ingest_staging_bytes(uint32_t w, uint32_t h, uint32_t pixels);
/* Decoded surfaces that already sit in device memory -> BGRA8 frames that smhv_batch_run, smhv_pipeline_submit and
 * smhv_load_frame_device take.  d_src = n frames, frame_stride bytes apart, each with its Y plane at offset 0 (rows y_pitch
 * apart), its U plane (NV12: the U, V pairs) at u_offset and, for I420, its V plane at v_offset (chroma rows uv_pitch apart);
 * bases and pitches may have any byte alignment.  layout = NULL, or a zero member, means tight: y_pitch = w, uv_pitch = 2 cw
 * (NV12) / cw (I420), u_offset = y_pitch * h, v_offset = u_offset + uv_pitch * ch, frame_stride = the end of the last plane.
 * `pixels` = SMHV_PIXELS_YUV(...).  d_bgra (4-byte aligned) receives n frames of w * h * 4 bytes with tight rows,
 * out_stride_bytes apart (a multiple of 4; 0 = w * h * 4).  flags: SMHV_YUV_ROI_ONLY writes the map ROI's and the button's
 * rectangles alone (smhv_map_bounds / smhv_button_bounds; the bytes of the full conversion) and leaves everything else in d_bgra
 * as it was.  Asynchronous on `stream` (NULL: the context's own).  SMHV_E_INVALID, with nothing enqueued, for a null pointer,
 * n, w or h = 0, a pitch shorter than its row, planes of a frame that reach beyond frame_stride when n > 1, an out_stride_bytes
 * shorter than a frame, an unknown layout or colour bit, or an unknown flag. */
typedef struct {
	uint64_t y_pitch, uv_pitch, u_offset, v_offset, frame_stride;
} smhv_yuv_layout;
#define SMHV_YUV_ROI_ONLY 1u
SMHV_API int smhv_yuv_to_bgra_device(smhv_ctx *ctx, const void *d_src, const smhv_yuv_layout *layout, uint32_t n, uint32_t w, uint32_t h, uint32_t pixels,
                                     void *d_bgra, uint64_t out_stride_bytes, uint32_t flags, void *stream);
/* ---- video frames OUT: RGBA8 / BGRA8 images -> NV12 / I420, what a hardware encoder takes ----------------------------------------
 * The output word is SMHV_PIXELS_YUV(layout, matrix, range, 0): the layouts, the matrix bit and the range bit of the inbound
 * direction.  The chroma bit must be 0 on output -- chroma is always the centre-sited 2 x 2 box -- and a set chroma bit, like
 * any other bit, is SMHV_E_INVALID.  For a source of w x h, cw = (w + 1) / 2 and ch = (h + 1) / 2 (odd sizes are legal).
 * The arithmetic, in int32 with >> the arithmetic shift; alpha is ignored:
 *   Y[y][x]   = clip8(((yr * R + yg * G + yb * B + 32768) >> 16) + yoff)
 *   Rs, Gs, Bs = the sums over the four pixels (min(2 cx + i, w - 1), min(2 cy + j, h - 1)), i, j in {0, 1}
 *                (at an odd edge a pixel counts twice: always four terms)
 *   U[cy][cx] = clip8(((ur * Rs + ug * Gs + ub * Bs + 131072) >> 18) + 128)
 *   V[cy][cx] = clip8(((vr * Rs + vg * Gs + vb * Bs + 131072) >> 18) + 128)
 * with (the real matrices times 65536, rounded; the green one of each row chosen so that yr + yg + yb is exactly 56284 (limited)
 * or 65536 (full) and ur + ug + ub = vr + vg + vb = 0)
 *                    yr     yg    yb  yoff     ur      ug     ub     vr      vg     vb
 *   709 limited   11966  40254  4064   16   -6596  -22188  28784  28784  -26145  -2639
 *   709 full      13933  46871  4732    0   -7509  -25259  32768  32768  -29763  -3005
 *   601 limited   16829  33039  6416   16   -9714  -19070  28784  28784  -24103  -4681
 *   601 full      19595  38470  7471    0  -11058  -21710  32768  32768  -27439  -5329
 * Grey pixels: R = G = B = l gives Y = clip8(((T * l + 32768) >> 16) + yoff) with T = 56284 (limited) or 65536 (full), and
 * U = V = 128 exactly -- so a grey image that is held as one luma byte per pixel converts without ever becoming RGBA.
 * Range: the largest product is 32768 * 1020 < 2^31, so int32 suffices; U reaches 256 in full range (saturated blue), so
 * clip8 is needed.  Y is within 1 level of the rounded float64 matrix for every colour, U and V within 1 level.
 *
 * smhv_bgra_to_yuv_device, the inverse of smhv_yuv_to_bgra_device: n images in device memory (d_src 4-byte aligned, rows
 * src_pitch_bytes apart: 0 = 4 w, a multiple of 4; images src_stride_bytes apart: 0 = src_pitch_bytes * h, a multiple of 4;
 * bytes B, G, R, A, or R, G, B, A with SMHV_VIDEO_SRC_RGBA in src_flags) -> n frames at d_dst laid out by `layout` as
 * smhv_yuv_layout describes them above (NULL or a zero member: tight).  Destination bases and pitches may have any byte
 * alignment; nothing but the planes' samples is written (pitch padding, gaps and what lies between frames keep their bytes).
 * Asynchronous on `stream` (NULL: the context's own).  SMHV_E_INVALID, with nothing enqueued, for a null pointer, n, w or h = 0,
 * a pitch shorter than its row, planes of a frame that reach beyond frame_stride when n > 1, a non-zero v_offset for NV12
 * (other than u_offset + 1), an unknown layout, colour bit or flag. */
#define SMHV_VIDEO_SRC_RGBA 1u
SMHV_API int smhv_bgra_to_yuv_device(smhv_ctx *ctx, const void *d_src, uint64_t src_pitch_bytes, uint64_t src_stride_bytes, uint32_t n, uint32_t w, uint32_t h,
                                     uint32_t src_flags, uint32_t pixels, void *d_dst, const smhv_yuv_layout *layout, void *stream);
/* What a batch shows a viewer, as video frames: frames [first, first + n) of `source` -> n frames at d_dst (`pixels`, `layout` as
 * above).  A call of its own, like the feed: no stage bit.  It reads what is in memory when `stream` reaches the call and works on
 * a plain batch and on a pipeline slot's batch after smhv_pipeline_wait.
 *   SMHV_VIDEO_RENDER: the render slab at the window size of the most recent render (smhv_batch_render_size);
 *                      SMHV_E_STATE before the first render.
 *   SMHV_VIDEO_UI_MAP: the ui_map at the ROI's size (smhv_map_bounds); SMHV_E_STATE when no run has produced one.  Per frame,
 *                      on the device, the kernel reads the form that holds the frame's newest ui_map: the luma plane of a grey
 *                      run (by the grey formula above: no RGBA is made, and the batch's state is left as it is) or the RGBA slab.
 *                      A frame a run found closed keeps its older image, in whichever form holds it. */
#define SMHV_VIDEO_RENDER 0u
#define SMHV_VIDEO_UI_MAP 1u
SMHV_API int smhv_batch_video(smhv_batch *b, uint32_t source, uint32_t first, uint32_t n, uint32_t pixels, void *d_dst, const smhv_yuv_layout *layout, void *stream);
/* the tight size of a frame of w x h in `pixels` (an output word): w h + 2 cw ch = smhv_ingest_staging_bytes of the same word;
   0 for a zero size or a word that is not an output word.  Needs no device. */
SMHV_API uint64_t smhv_video_bytes(uint32_t w, uint32_t h, uint32_t pixels);
/* wait for everything committed (or until the slab is full); *d_frames = slab of *n <= capacity accepted frames, valid
 * until smhv_ingest_reset; *last_crc (optional) = CRC-32 of the last accepted frame.  Frames committed after the slab
 * filled up are not lost: they stay queued in their staging slots (at most `slots` of them -- smhv_ingest_acquire
 * returns SMHV_E_STATE when the slab is full and no slot is free) and go into the next slab after smhv_ingest_reset. */
SMHV_API int smhv_ingest_batch(smhv_ingest *q, const void **d_frames, uint32_t *n, uint32_t *last_crc);
/* start a new slab (the consumer of the previous one must have finished with it); the duplicate test keeps comparing
 * with the last accepted frame; frames still queued are resolved into the new slab by the next acquire / batch */
SMHV_API int smhv_ingest_reset(smhv_ingest *q);
SMHV_API int smhv_ingest_counts(smhv_ingest *q, uint64_t *n_new, uint64_t *n_dup);
/* CRC-32/IEEE of nbytes of HOST memory (any length, any alignment; PCLMULQDQ folding where the CPU has it); needs no device */
SMHV_API uint32_t smhv_crc32_host(const void *data, uint64_t nbytes);
/* CRC-32/IEEE of nbytes (multiple of 4) of device memory; == crc32fast::hash / zlib crc32 of the same bytes */
SMHV_API int smhv_crc32_device(smhv_ctx *ctx, const void *d_data, uint64_t nbytes, uint32_t *crc);

/* ---- firing solutions: range, altitude difference, mils and bearings of every marker line -----------------------------
 * The numbers the app draws beside a marker (src/ui/markers.rs:23-200): the range from the heightmap and the minimap rectangle
 * when a heightmap is bound (markers.rs:37-91), else from the map scales (the record's meters); the altitude difference between
 * the two ends (Heightmap::height, heightmap-ripper/src/lib.rs:22-25); the elevation in milliradians for each direction
 * (src/squadex/milliradians.rs) and the bearing for each direction (markers.rs:98-110).  Per line (p0, p1) in map-ROI
 * coordinates, with Rust's f32 / f64 semantics:
 *   P = (x * sw + tx, y * sh + ty) in f32 (the viewport, src/ui/map.rs:80-101; default sw = sh = 1, tx = ty = 0).
 *   Heightmap branch (the frame has a minimap rectangle and a heightmap is bound): offset = (0, 0) ("fit to minimap", the app's
 *   default), or with SMHV_FIRING_BOUNDS_OFFSET  off.x = b0.x * ((right - left) as f32 / (W as f32 + b0.x)) * sw, the same in y
 *   (b0 = bounds[0] as f32, right - left in u32).  R = {left*sw+tx + off.x, top*sh+ty + off.y, right*sw+tx, bottom*sh+ty} in f32;
 *   p_x = ((P.x as f64 - R.left as f64) / (R.right - R.left) as f64) * W, the same in y; range = sqrt(dx*dx + dy*dy) in f64.  The
 *   four coordinates are rounded half away from zero and cast `as i32` (saturating, NaN -> 0): if all lie inside [0,W) x [0,H),
 *   alt_delta = height(p1) - height(p0) with height = (v as f64 / 65535.0) * (scale[2] as f64 / 0.1953125); otherwise the
 *   heightmap gives no range.
 *   Range: the heightmap's, else the record's meters when the frame has m/px, else none (source says which).
 *   Bearings: angle = atan2f(P0.y - P1.y, P0.x - P1.x), d = angle * 57.29578 (f32 to_degrees); d > 0 ? (d -= 90, d < 0 ? d += 360)
 *   : d += 270; fwd = roundf(d) fmod 360, bck = roundf(fwd + 180) fmod 360 (roundf: half away from zero).
 *   Mils: calc(m, a) = atan((V^2 + sqrt(V^4 - g(g m m + 2 a V^2))) / (g m)) * (180 / pi) / (360 / 6400) in f64, g = 9.8,
 *   V = 109.890938; NaN = out of range (the app's "RANGE!").
 * Directions: [0] = firing from p0 at p1 (alt_delta = height(p1) - height(p0), mils[0] = calc(range, alt_delta), bearing[0] =
 * fwd); [1] = the reverse (mils[1] = calc(range, -alt_delta), bearing[1] = bck).  Without alt_delta both mils are calc(range, 0).
 * What the app prints where (markers.rs:131, :202), angle as above:
 *   with alt_delta (source HEIGHTMAP): the text left of the midpoint ("<- ... mil") is direction 0 when -pi/2 <= angle < pi/2 and
 *     direction 1 otherwise; the text right of it ("... mil ->") is the other direction.
 *   without (source SCALES): one block; when -pi/2 <= angle <= pi/2 its lines read "-> bearing[1]" then "<- bearing[0]", otherwise
 *     "-> bearing[0]" then "<- bearing[1]".
 *   source NONE: the app draws the line only (the bearings are filled all the same; meters, alt_delta and mils are 0). */
typedef struct smhv_heightmap smhv_heightmap;
#define SMHV_STAGE_FIRING 0x80u          /* smhv_batch_run / smhv_pipeline_submit: write the firing slab (needs SMHV_STAGE_MARKERS; the
                                            heightmap branch needs SMHV_STAGE_MINIMAP in the same run -- without it every line takes
                                            the scales branch, as the reference does without minimap bounds).  Not in SMHV_STAGE_ALL. */
#define SMHV_FIRING_BOUNDS_OFFSET 1u     /* smhv_firing_options.flags: the app's "fit to minimap" switched off (bounds[0] offsets the map) */
#define SMHV_FIRING_NONE 0u              /* smhv_firing.source */
#define SMHV_FIRING_SCALES 1u
#define SMHV_FIRING_HEIGHTMAP 2u
typedef struct {
	uint32_t size;                       /* sizeof(smhv_firing_options) */
	uint32_t flags;                      /* SMHV_FIRING_* */
	float viewport_scale[2];             /* MapViewport::scale_factor_{w,h}; 0 = 1 */
	float viewport_top_left[2];          /* MapViewport::top_left */
} smhv_firing_options;
typedef struct {
	double meters;                       /* range (0 when source is NONE)                                   */
	double alt_delta;                    /* height(p1) - height(p0) (source HEIGHTMAP; 0 otherwise)          */
	double mils[2];                      /* [0] from p0 at p1, [1] from p1 at p0; NaN = out of range          */
	float bearing[2];                    /* degrees, [0] = fwd, [1] = bck                                     */
	uint32_t source;                     /* SMHV_FIRING_NONE / _SCALES / _HEIGHTMAP                          */
	uint32_t reserved;
} smhv_firing;
typedef struct {
	uint32_t n_lines, reserved;          /* == the record's n_lines; lines beyond it are zero                 */
	smhv_firing line[SMHV_MAX_LINES];
} smhv_firing_result;
/* A device copy of a heightmap (Heightmap, heightmap-ripper/src/lib.rs:7-14): w x h u16 texels, row-major; bounds = {b00, b01,
 * b10, b11}; scale = {x, y, z}.  SMHV_E_INVALID for a zero dimension or w*h > 2^28.  smhv_heightmap_destroy drops the caller's
 * reference: a batch or pipeline that has it bound keeps its own until it is rebound or destroyed, and the device memory goes
 * with the last reference once the device has finished everything enqueued before (that release synchronises the device). */
SMHV_API int smhv_heightmap_create(smhv_ctx *ctx, const uint16_t *data, uint32_t w, uint32_t h, const int32_t bounds[4], const float scale[3],
                                   smhv_heightmap **out);
SMHV_API void smhv_heightmap_destroy(smhv_heightmap *hm);
/* color_map_heightmap (src/ui/heightmaps.rs:169-207): w*h*4 bytes of RGBA into host memory, byte-exact (a min/max pass, then the
 * per-texel colour in f64) */
SMHV_API int smhv_heightmap_color_map(smhv_heightmap *hm, uint8_t *rgba);
/* Bind a heightmap (NULL = none) and options (NULL = defaults) for SMHV_STAGE_FIRING.  A batch's binding applies to its next
 * smhv_batch_run; a pipeline's to submissions made after the call (submissions in flight keep what they were submitted with). */
SMHV_API int smhv_batch_set_firing(smhv_batch *b, smhv_heightmap *hm, const smhv_firing_options *opt);
SMHV_API int smhv_pipeline_set_firing(smhv_pipeline *p, smhv_heightmap *hm, const smhv_firing_options *opt);
/* The batch's firing slab: one smhv_firing_result per frame, written by runs with SMHV_STAGE_FIRING (allocated by the first
 * such run).  read: synchronising host copy; ptr: device address (SMHV_E_STATE before the first such run). */
SMHV_API int smhv_batch_read_firing(smhv_batch *b, uint32_t first, uint32_t n, smhv_firing_result *out);
SMHV_API int smhv_batch_firing_ptr(smhv_batch *b, void **d_firing);
/* The same device function for explicit lines (markers::draw of detected and custom markers): n lines in map-ROI coordinates,
 * mpx = the frame's meters per pixel (NULL: none), minimap = {left, right, top, bottom} (NULL: none), hm (NULL: none), opt (NULL:
 * defaults).  Runs on the context's stream and returns the n results. */
SMHV_API int smhv_firing_solutions(smhv_ctx *ctx, const smhv_line *lines, uint32_t n, const double *mpx, const uint32_t minimap[4],
                                   const smhv_heightmap *hm, const smhv_firing_options *opt, smhv_firing *out);

/* ---- heightmap overlay: the colour map drawn over the minimap --------------------------------------------------------
 * The picture the app shows when a heightmap is lined up with the minimap: the ui_map drawn with nearest filtering
 * (src/ui/map.rs:250-256), then the heightmap's colour map stretched over the minimap rectangle with linear filtering, tinted
 * [1, 1, 1, 0.25] (heightmaps::render_overlay, src/ui/heightmaps.rs:794-826).  The output is an image in ui_map pixel space: the
 * ui_map as the app shows it at viewport scale 1, w x h RGBA8.  The viewport fields of smhv_firing_options do not apply to it;
 * only flags does (SMHV_FIRING_BOUNDS_OFFSET = "fit to minimap" off).  GL rasterisation and filtering are not bit-reproducible,
 * so the library pins one exact restatement of the draw: every operation f32, left to right, unfused.  Inputs: U = the frame's
 * ui_map (w x h RGBA8, grayscale or colour as the run produced it); mm = {left, right, top, bottom}, the frame's minimap
 * rectangle (u32); C = the colour map, W x H RGBA8, byte-equal to smhv_heightmap_color_map; b00, b01 = bounds[0], bounds[1] as f32.
 *   1. Offset: (0, 0) ("fit", the default); with SMHV_FIRING_BOUNDS_OFFSET off.x = b00 * ((float)(right - left) / ((float)W + b00)),
 *      off.y = b01 * ((float)(bottom - top) / ((float)H + b01)) (heightmaps.rs:802-808 at scale 1; right - left in u32).
 *   2. Quad (imgui's Image at the cursor, bottom right = min + size): x0 = (float)left + off.x, y0 = (float)top + off.y,
 *      sx = (float)right - x0, sy = (float)bottom - y0, x1 = x0 + sx, y1 = y0 + sy.
 *   3. Coverage: pixel (x, y) of U, centre cx = x + 0.5f, cy = y + 0.5f, is covered iff x0 <= cx && cx < x1 && y0 <= cy && cy < y1
 *      (half-open; NaN compares false, so W + b00 == 0 or a degenerate quad covers nothing).  Only pixels inside U are written.
 *   4. Sampling (GL_LINEAR, no mipmaps): s = ((cx - x0) / sx) * (float)W - 0.5f, i = floorf(s), fx = s - i; t = ((cy - y0) / sy) *
 *      (float)H - 0.5f, j = floorf(t), fy = t - j.  Taps i, i+1 and j, j+1, each clamped to the image (clamp to edge: for texture
 *      coordinates in [0, 1] clamp and mirrored wrap give the same taps; this library states clamp).  Per channel, C as f32 in
 *      0..255, gx = 1.0f - fx, gy = 1.0f - fy: top = C[j][i]*gx + C[j][i+1]*fx, bot = C[j+1][i]*gx + C[j+1][i+1]*fx, c = top*gy + bot*fy.
 *   5. Blend (imgui's alpha blending; the tint alpha as imgui stores it, 0.25f * 255 + 0.5 truncated = 64; every colour-map texel
 *      is opaque): A = 64.0f / 255.0f, B = 1.0f - A; for R, G, B  o = c*A + u*B (u = U's channel), byte = (uint8_t)fminf(o + 0.5f,
 *      255.0f); alpha = 255.
 *   6. Uncovered pixels keep U's bytes; an open frame without a minimap rectangle is U unchanged (the app draws no overlay then,
 *      heightmaps.rs:797). */
#define SMHV_STAGE_HEIGHTMAP_OVERLAY 0x100u /* smhv_batch_run / smhv_pipeline_submit: write the overlay slab.  Needs SMHV_STAGE_UI_MAP,
                                               SMHV_STAGE_MINIMAP and a heightmap bound with smhv_batch_set_firing /
                                               smhv_pipeline_set_firing (the same binding and rule as SMHV_STAGE_FIRING); without them
                                               the call returns SMHV_E_INVALID and enqueues nothing.  Not in SMHV_STAGE_ALL.  The
                                               heightmap's colour table is built by its first overlay (that call synchronises once). */
#define SMHV_IMAGE_HEIGHTMAP_OVERLAY 101 /* smhv_batch_read_image: the overlay of a frame, w x h RGBA8 (100 = the ui_map) */
/* The batch's overlay slab: one image per frame with the ui slab's layout (smhv_batch_layout ui_pitch / ui_stride / ui_offset),
 * allocated by the first run with SMHV_STAGE_HEIGHTMAP_OVERLAY; such a run writes every open frame and leaves closed frames alone.
 * Device address (SMHV_E_STATE before the first such run; so is smhv_batch_read_image with SMHV_IMAGE_HEIGHTMAP_OVERLAY). */
SMHV_API int smhv_batch_overlay_ptr(smhv_batch *b, void **d_overlay);
/* The per-call path: the overlay of the context's current frame -- the ui_map smhv_crop_to_map left on the device and the rectangle
 * its walk found (what smhv_find_minimap returns) -- w x h RGBA8 into host memory.  hm required, opt NULL = defaults.  On the
 * context's stream; SMHV_E_INVALID before load_frame / crop_to_map, SMHV_E_STATE when the map is closed. */
SMHV_API int smhv_heightmap_overlay(smhv_ctx *ctx, const smhv_heightmap *hm, const smhv_firing_options *opt, uint8_t *rgba);

/* ---- map view: what the app's window shows, at any viewport ------------------------------------------------------------
 * map::render (src/ui/map.rs:209-273) draws, in this order: the ui_map as a quad placed by MapViewport::calc (letter-boxed into
 * the window, zoomed, panned; nearest filtering, map.rs:180-199, 250-254), the heightmap overlay through that viewport
 * (heightmaps.rs:794-826), then every marker line (markers.rs:28-30, thickness 2, colours map.rs:260-267).  A render call draws
 * that picture on the device from results that are already there -- the ui slab and the records -- into the batch's render
 * slab: out_w x out_h RGBA8 per frame, tightly packed.  The viewport belongs to the display loop, not to the vision loop, so this
 * is a call of its own and no stage bit; it works the same after smhv_pipeline_wait on a slot's batch, for both searches.
 * GL's and imgui's rasterisation are not bit-reproducible, so, as for the overlay, the library pins ONE exact restatement: every
 * operation one f32 operation, left to right, unfused.  Output pixel (X, Y), centre cx = X + 0.5f, cy = Y + 0.5f in window
 * coordinates; U = the frame's ui_map (w x h), rec = its record; {ql, qt, qr, qb} = quad; sw, sh = viewport_scale (0 means 1, as
 * in smhv_firing_options); tx, ty = viewport_top_left.
 *   0. o = background.  A frame whose map is closed is background everywhere (the slab never keeps stale pixels).
 *   1. Map quad: covered iff ql <= cx && cx < qr && qt <= cy && cy < qb (half-open; NaN covers nothing).
 *      u = ((cx - ql) / (qr - ql)) * (float)w, ix = clamp((int)floorf(u), 0, w - 1); v = ((cy - qt) / (qb - qt)) * (float)h,
 *      iy = clamp((int)floorf(v), 0, h - 1); o = U[iy][ix] (R, G, B; alpha 255).
 *   2. Overlay (SMHV_RENDER_HEIGHTMAP, rec.has_minimap): R = the heightmap's rectangle WITH the viewport, exactly the firing
 *      solutions' (see there): off = (0, 0), or with SMHV_RENDER_BOUNDS_OFFSET off.x = b00 * ((float)(right - left) / ((float)W +
 *      b00)) * sw, the same in y; R = {(left*sw + tx) + off.x, (top*sh + ty) + off.y, right*sw + tx, bottom*sh + ty}.  Then steps
 *      2-5 of the overlay above with x0 = R.left, y0 = R.top, sx = R.right - x0, sy = R.bottom - y0 (x1 = x0 + sx, y1 = y0 + sy)
 *      and `o` in the place of the ui_map pixel u; alpha 255.  Coverage does not depend on step 1: the overlay is also drawn
 *      over the background.
 *   3. Marker lines (SMHV_RENDER_MARKERS): line i of n (rec.lines / rec.n_lines, or the explicit ones): P = (x * sw + tx,
 *      y * sh + ty) for both ends; dx = P1.x - P0.x, dy = P1.y - P0.y; len2 = dx*dx + dy*dy; skipped unless len2 > 0.
 *      ax = cx - P0.x, ay = cy - P0.y; t = ax*dx + ay*dy; c = ax*dy - ay*dx.  Painted iff 0 <= t && t <= len2 && c*c <= len2
 *      (the centre within 1.0 of the segment, butt ends; no square root).  f = (float)(i + 1) / (float)n; r = (uint8_t)((1.0f -
 *      f) * 255.0f + 0.5f), g = (uint8_t)(f * 255.0f + 0.5f), b = 0, alpha 255.  Later lines paint over earlier ones.  This is
 *      a HARD-EDGED stroke in the place of imgui's anti-aliased one.  Text labels are not drawn by this call: they are a pass of their own
 *      over its image, smhv_batch_render_labels / smhv_render_map_labeled ("map view: labels").
 * Two identities follow: with out = (w, h), quad = {0, 0, w, h}, scale 1, top left 0 and no flags the image is the ui_map; with
 * SMHV_RENDER_HEIGHTMAP added it is SMHV_STAGE_HEIGHTMAP_OVERLAY's image of the same heightmap, byte for byte. */
#define SMHV_RENDER_HEIGHTMAP 1u       /* smhv_render_options.flags: draw the heightmap overlay (needs hm) */
#define SMHV_RENDER_MARKERS 2u         /*   ... the marker lines */
#define SMHV_RENDER_BOUNDS_OFFSET 4u   /*   ... the app's "fit to minimap" switched off (as SMHV_FIRING_BOUNDS_OFFSET) */
#define SMHV_RENDER_MAX_LINES 256u     /* explicit lines of one smhv_render_map call */
typedef struct {
	uint32_t size;                       /* sizeof(smhv_render_options) */
	uint32_t flags;                      /* SMHV_RENDER_* */
	uint32_t out_w, out_h;               /* the window (display_size), in pixels; at most 16384 each */
	float quad[4];                       /* {left, top, right, bottom}: the Rect MapViewport::calc returns */
	float viewport_scale[2];             /* MapViewport::scale_factor_{w,h}; 0 = 1 */
	float viewport_top_left[2];          /* MapViewport::top_left */
	uint8_t background[4];               /* RGBA of pixels nothing is drawn on */
} smhv_render_options;
/* MapViewport::calc (src/ui/map.rs:21-77) in f32; host only, needs no device.  region = the window, map = the ui_map's size,
 * zoom = the wheel's level (0 = none; levels above 10 zoom as 10), zoom_pos / pan_pos may be NULL (0, 0).  Fills opt->quad,
 * opt->viewport_scale and opt->viewport_top_left and nothing else -- the two viewport fields are what smhv_firing_options takes,
 * so the numbers and the picture use one viewport. */
SMHV_API int smhv_map_viewport_calc(float region_w, float region_h, float map_w, float map_h, uint32_t zoom, const float zoom_pos[2],
                                    const float pan_pos[2], smhv_render_options *opt);
/* Draws frames [first, first + n) of the batch from the ui slab and the records as they are when `stream` reaches this point;
 * asynchronous, on `stream`.  The image of frame f lies at d_images + f * stride of the render slab.  The slab holds the batch's
 * whole capacity at the window's size (capacity * out_w * out_h * 4 bytes), so a batch may be rendered in parts.  It is allocated
 * by the first render and re-allocated when a later one asks for a larger window: that call waits (host) for the batch's previous
 * render and frees the old slab, which waits for the device to run dry; pointers handed out before are stale then and the earlier
 * images are gone (frames the renders since have not drawn hold undefined bytes).  A render at another window size of equal or
 * fewer bytes re-uses the slab with the new stride: images of the previous size are not readable any more.  SMHV_E_INVALID: a zero or too large out_w / out_h, a size mismatch, unknown flags, n == 0 or first + n beyond the
 * batch's capacity, SMHV_RENDER_HEIGHTMAP without hm, a quad edge that is not finite (MapViewport::calc produces none from finite arguments);
 * SMHV_E_STATE: no run of the batch has produced a ui_map.  A failed call
 * enqueues nothing.  The batch keeps a reference of hm until a later render takes another heightmap or the batch is destroyed,
 * so the caller may drop its own right after the call.  The heightmap's colour table is built by its first overlay or render
 * (that call waits for it once, on a stream of its own). */
SMHV_API int smhv_batch_render(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *opt, void *stream);
/* the render slab and its per-frame stride, out_w * out_h * 4, of the most recent render (SMHV_E_STATE before the first) */
SMHV_API int smhv_batch_render_ptr(smhv_batch *b, void **d_images, uint64_t *stride);
/* the window of the most recent render (SMHV_E_STATE before the first): what smhv_batch_read_render copies per frame */
SMHV_API int smhv_batch_render_size(smhv_batch *b, uint32_t *out_w, uint32_t *out_h);
/* synchronising host copy of one frame's image as the most recent render sized it (out_w * out_h * 4 bytes) */
SMHV_API int smhv_batch_read_render(smhv_batch *b, uint32_t frame, uint8_t *rgba);
/* The per-call path: the context's current frame -- the ui_map smhv_crop_to_map left on the device, the rectangle its walk found --
 * and explicit lines in map-ROI coordinates (detected and custom markers; n_lines <= SMHV_RENDER_MAX_LINES), out_w x out_h RGBA8
 * into host memory.  On the context's stream; SMHV_E_INVALID before load_frame / crop_to_map, SMHV_E_STATE when the map is closed.
 * The image crosses in one piece through pinned staging of the context, which grows to the largest window rendered and stays
 * (out_w * out_h * 4 bytes: 14 MB at 2560 x 1440; the 16384 limit would pin 1 GiB -- windows of that size belong to smhv_batch_render). */
SMHV_API int smhv_render_map(smhv_ctx *ctx, const smhv_heightmap *hm, const smhv_render_options *opt, const smhv_line *lines, uint32_t n_lines,
                             uint8_t *rgba);

/* ---- map view: layers -- custom markers, the Debug menu's overlays, a debug view as the map ---------------------------------
 * What the reference's window shows beside the three layers above: draw::render (src/ui/draw.rs:135-198) draws the user's custom
 * markers and the marker being dragged in magenta and the measuring line in red BEFORE the detected markers (map.rs:258 runs
 * before map.rs:260-270); the Debug menu (src/ui/debug.rs:286-345) puts OCR boxes (1 px outlines), the computed scale bars (2 px
 * lines) and the minimap bounds (a 1 px outline, shifted by one pixel) on the foreground draw list, above everything; and
 * map::render starts with debug_view.unwrap_or(map) (map.rs:210): a debug view can be the map quad's texture.  The two calls below
 * draw the map view with these layers; smhv_batch_render / smhv_render_map are unchanged and keep their kernels.  Every operation
 * one f32 operation, left to right, unfused; cx, cy, sw, sh, tx, ty as in the map view.
 *   0. Background: unchanged.  A closed frame is background everywhere.
 *   1. Map quad: with map_source != SMHV_VIEW_NONE step 1 samples that image, at its own width and height, in the place of U, w, h.
 *      Nothing else changes: the overlay, the lines and the prims stay in map-ROI coordinates through the same viewport, as the
 *      reference does when a quadrant view is the map.
 *   2. Overlay: unchanged.
 *   3. Paint order, later over earlier: (1) prims without SMHV_PRIM_FOREGROUND, in list order; (2) the detected marker lines
 *      (SMHV_RENDER_MARKERS: exactly the map view's rule and colours, f = (i + 1) / n over the lines alone); (3) prims with
 *      SMHV_PRIM_FOREGROUND, in list order; (4) the minimap bounds.
 *      A prim's end points: P0 = (x0 * sw + tx, y0 * sh + ty), P1 likewise; with SMHV_PRIM_SHIFT1 1.0f is then added to all four
 *      values.  Colour = rgba[0..2], alpha 255.
 *      SMHV_PRIM_LINE: the map view's stroke: dx = P1.x - P0.x, dy = P1.y - P0.y, len2 = dx*dx + dy*dy, skipped unless len2 > 0;
 *      painted iff 0 <= t && t <= len2 && c*c <= len2.
 *      SMHV_PRIM_RECT: a = (fminf(P0.x, P1.x), fminf(P0.y, P1.y)), b = (fmaxf(P0.x, P1.x), fmaxf(P0.y, P1.y)) -- a NaN operand yields
 *      the other one.  Painted iff a.x <= cx && cx < b.x && a.y <= cy && cy < b.y and not (a.x + 1.0f <= cx && cx < b.x - 1.0f &&
 *      a.y + 1.0f <= cy && cy < b.y - 1.0f): a HARD-EDGED 1 px frame in the place of imgui's stroke of the rectangle [a + 0.5,
 *      b - 0.5] with thickness 1.  A rectangle narrower or flatter than 2 is filled; a degenerate or NaN one paints nothing.
 *      SMHV_LAYER_MINIMAP_BOUNDS: when rec.has_minimap, a RECT with corners ((float)left, (float)top), ((float)right, (float)bottom)
 *      with SMHV_PRIM_SHIFT1 (debug.rs:326-329), colour (0, 255, 0); without a rectangle nothing.  The reference's text is not drawn here (the
 *      marker labels are "map view: labels", the Debug menu's text is "map view: debug text and the vision debugger").
 * Two identities: with n_prims = 0, flags = 0 and map_source = SMHV_VIEW_NONE the image is smhv_batch_render's / smhv_render_map's,
 * byte for byte; with the identity viewport at the view's size and nothing else the image is the view (smhv_get_debug_view's on the
 * per-call path).
 * Map sources.  Per call: U is exactly what smhv_get_debug_view(ctx, which, ...) returns at that moment, under its state rules.
 * Batch: sampled in the kernel from the slabs the run left (nothing the size of a batch is materialised):
 *   SMHV_VIEW_OCR_INPUT, SMHV_VIEW_FIND_SCALES_INPUT   (L, L, L, 255) from the ocr / scales slab, brq_w x brq_h
 *   SMHV_VIEW_LSD_INPUT                                (L, L, L, 255) from the mask slab, w x h
 *   SMHV_VIEW_LSD_PREPROCESS   the colour ui_map with every pixel that fails the marker predicate (0, 0, 0), alpha 255 (the batch
 *                              always isolates), w x h
 *   SMHV_VIEW_CROPPED_BRQ      pixel (x, y) = the colour ui_map's (x + w/2, y + h/2), w/2 x h/2
 * A batch (a pipeline slot's too) remembers which of these its runs have produced: SMHV_E_STATE when no run had the OCR / SCALES
 * (with anchors) / MARKERS stage for the first three, or when the ui_map is missing or the last one written is grayscale for the
 * last two. */
#define SMHV_PRIM_LINE        0u      /* kind, low byte: a 2 px stroke, the rule of step 3 of the map view            */
#define SMHV_PRIM_RECT        1u      /*                 a 1 px rectangle outline with corners (x0, y0), (x1, y1)     */
#define SMHV_PRIM_FOREGROUND  0x100u  /* painted above the detected markers (the foreground draw list); without it:
                                         below them (draw::render)                                                     */
#define SMHV_PRIM_SHIFT1      0x200u  /* 1.0f is added to both translated corners (debug.rs:326-329)                  */
#define SMHV_RENDER_MAX_PRIMS 256u
typedef struct { float x0, y0, x1, y1; uint8_t rgba[4]; uint32_t kind; } smhv_render_prim;   /* 24 bytes; map-ROI coordinates */

#define SMHV_LAYER_MINIMAP_BOUNDS 1u  /* smhv_render_layers.flags: the record's minimap rectangle, drawn by the device */
typedef struct {
	uint32_t size;                     /* sizeof(smhv_render_layers) */
	uint32_t flags;                    /* SMHV_LAYER_* */
	uint32_t map_source;               /* SMHV_VIEW_NONE = the ui_map, or a SMHV_VIEW_*: that image is the map quad's texture */
	uint32_t n_prims;                  /* <= SMHV_RENDER_MAX_PRIMS */
	const smhv_render_prim *prims;     /* host memory; copied before the call returns; the same list for every frame of the call */
} smhv_render_layers;
/* smhv_batch_render with layers: the same slab, growth, stride and read rules, asynchronous on `stream`.  The prims cross through
 * pinned staging of the batch: a call with prims waits (host) until the previous call's copy of them has run.  Errors as
 * smhv_batch_render, and SMHV_E_INVALID for a wrong size, unknown flags, an unknown kind or unknown kind bits, an unknown map_source,
 * n_prims > SMHV_RENDER_MAX_PRIMS, n_prims != 0 with prims == NULL, a prim whose rgba[3] != 255; SMHV_E_STATE when the chosen source
 * is not there.  A failed call enqueues nothing. */
SMHV_API int smhv_batch_render_layers(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *opt,
                                      const smhv_render_layers *layers, void *stream);
/* smhv_render_map with layers: host memory through the context's pinned staging, synchronous.  Errors as smhv_render_map and as above. */
SMHV_API int smhv_render_map_layers(smhv_ctx *ctx, const smhv_heightmap *hm, const smhv_render_options *opt, const smhv_render_layers *layers,
                                    const smhv_line *lines, uint32_t n_lines, uint8_t *rgba);

/* ---- map view: labels -- range, mils, bearings and altitude as text beside every marker line ------------------------------------
 * markers::draw (src/ui/markers.rs:93-211) prints the firing solution of a line as text that runs along the line and hangs below
 * its midpoint.  The calls below draw that text, as a pass of their own over a finished image of the map view, and hand out the
 * strings and their placement.  imgui's anti-aliased TTF text (Inter Bold, 20 px, src/ui/fonts/mod.rs:61) is not bit-reproducible,
 * so the library pins ONE hard-edged restatement, as the stroke rule does.  Every f32 operation is one operation, left to right,
 * unfused.
 * Font.  A 5 x 7 bitmap font drawn for this project (csrc/smh_font5x7.h: 7 row bytes per glyph, top row first, bit 4 = the leftmost
 *   column); nothing of the reference's TTF files is used.  A glyph sits in a 6 x 9 cell: the advance is 6 font units, the line
 *   height 9, the glyph occupies columns 0-4 and rows 1-7.  Exactly 27 glyphs: 0-9, m i l a t, R A N G E !, < - >, space, the
 *   plus-minus sign and the degree sign.  Strings are Latin-1 bytes (plus-minus 0xB1, degree 0xB0).  S = window pixels per font
 *   unit = smhv_label_options.scale, 1 .. 4, 0 means 2 (a glyph of 10 x 14 px, close to the reference's size).
 * Which lines, in which order (= slot order).  First the `extra` lines of the call in list order (custom markers, the drag, the
 *   measuring line: draw.rs:135-198), each with its own RGB.  Then, with SMHV_LABEL_DETECTED, the detected lines in order: in a
 *   batch rec.lines[0 .. n_lines), per call the explicit `lines` (at most SMHV_MAX_LINES); their colour is the map view's ramp,
 *   f = (i + 1) / n, the same bytes.  Later labels paint over earlier ones and all labels paint over everything already in the
 *   image.  THIS DEVIATES from the reference, where a later marker's stroke and the foreground draw list lie above an earlier
 *   marker's text: here the text always wins.
 * Numbers.  Every labelled line gets the firing solutions' device function (see "firing solutions": the same code
 *   smhv_firing_solutions runs, so picture and numbers cannot disagree; SMHV_STAGE_FIRING need not have run) with the render
 *   call's viewport_scale / viewport_top_left, SMHV_RENDER_BOUNDS_OFFSET as SMHV_FIRING_BOUNDS_OFFSET, the heightmap passed to the
 *   call (NULL: none), and the frame's minimap rectangle and m/px: in a batch the record's, per call the context's rectangle and
 *   smhv_label_options.mpx (NULL: none).  The record's-meters input of a detected line of a batch is rec.meters[i]; of every other
 *   line it is sqrt((double)(x0-x1)*(double)(x0-x1) + (double)(y0-y1)*(double)(y0-y1)) * mpx (Marker::new, ui/mod.rs:131-140), valid
 *   only when the frame has m/px.
 * No label (the slot stays, with n_runs = 0, mid = dir = 0): source == SMHV_FIRING_NONE; one of the four translated coordinates is
 *   not finite; len2 == 0; !(meters < 999999.5).
 * Strings (a release build's: the debug_assertions rows are not printed).  {:.0} of an f64 is rint() (ties to even) printed as an
 *   unsigned decimal; bearings are whole numbers already; A = |alt_delta as i32| with Rust's cast (truncating, saturating; the
 *   lower saturation gives 2147483648); mil(d) = "RANGE!" when mils[d] is NaN, else rint(mils[d]).  d = P0 - P1, the translated
 *   ends, in f32 (markers.rs:98).  "+-" and "deg" below stand for the bytes 0xB1 and 0xB0.
 *   Source SCALES, four rows: "{m}m"; "{mil(0)} mil" or "RANGE!"; then, if d.x >= 0, "-> {bearing[1]}deg" and "<- {bearing[0]}deg",
 *     otherwise "-> {bearing[0]}deg" and "<- {bearing[1]}deg" (d.x >= 0 is -pi/2 <= angle <= pi/2 in signs, markers.rs:202).
 *   Source HEIGHTMAP: the rows "{m}m" and "+-{A}m alt", a left block "<- {mil(a)} mil" (or "<- RANGE!"), "{bearing[a]}deg" and a
 *     right block "{mil(b)} mil ->" (or "RANGE! ->"), "{bearing[b]}deg"; a = 0, b = 1 when d.x > 0 || (d.x == 0 && d.y < 0) (-pi/2 <=
 *     angle < pi/2 in signs, markers.rs:131), otherwise a = 1, b = 0.  Run order: the two rows, the left block, the right block.
 * Layout, in HALF font units (all integers); row k is w_k = 6 * chars wide; a run is (x2, y2, text).
 *   SCALES: W2 = max(w_0, w_1), W4 = max(w_0 .. w_3); x2_k = -W2 + (W4 - w_k), y2_k = 18 k (markers.rs:199-210 with its quirk: the
 *     block is centred on the first two rows' width, each row in the width of all four).
 *   HEIGHTMAP: the two rows x2_k = -w_k, y2 = 0, 18.  Wf, Wb = the blocks' widest rows, G = 5 (the reference's 10 px): left-block
 *     rows, right-aligned, x2 = -(Wf + Wb + G) + 2 (Wf - w_k); right-block rows, left-aligned, x2 = -(Wf + Wb + G) + 2 (G + Wf); both
 *     blocks at y2 = 36, 54 (markers.rs:179-187).
 *   At most 6 runs of at most 16 characters.
 * Placement.  M = ((P0.x + P1.x) / 2, (P0.y + P1.y) / 2); len = sqrtf(d.x*d.x + d.y*d.y), correctly rounded; s = d.x > 0 ? 1 : -1;
 *   e = ((s*d.x) / len, (s*d.y) / len): text_angle (markers.rs:112-118, rotate.rs) without trigonometry -- along the line, never
 *   upside down, below the midpoint.
 * Pixel rule.  Pixel (X, Y), cx = X + 0.5f, cy = Y + 0.5f: ax = cx - M.x, ay = cy - M.y; u = (ax*e.x + ay*e.y) / (float)S;
 *   v = (ay*e.x - ax*e.y) / (float)S.  For each run iu = floorf(u - (float)x2 * 0.5f), iv = floorf(v - (float)y2 * 0.5f); the run is
 *   hit iff 0 <= iu < 6 * chars and 0 <= iv < 9; the pixel is painted iff the glyph of text[iu / 6] has its bit at column iu % 6
 *   (< 5) and row iv - 1 (0 .. 6).  Colour = the label's RGB, alpha 255.  A closed frame gets nothing (its result has n_labels = 0). */
#define SMHV_LABEL_DETECTED 1u        /* smhv_label_options.flags: label the detected lines too */
#define SMHV_LABEL_MAX_EXTRA 64u
typedef struct { smhv_line line; uint8_t rgba[4]; } smhv_label_line;          /* rgba[3] must be 255 */
typedef struct {
	uint32_t size;                       /* sizeof(smhv_label_options) */
	uint32_t flags;                      /* SMHV_LABEL_* */
	uint32_t scale;                      /* S: 1 .. 4, 0 = 2 */
	uint32_t n_extra;                    /* <= SMHV_LABEL_MAX_EXTRA */
	const smhv_label_line *extra;        /* host memory; copied before the call returns; the same list for every frame of the call */
	const double *mpx;                   /* the per-call path's meters per pixel (NULL: none); a batch takes the record's */
} smhv_label_options;
typedef struct { int16_t x2, y2; uint8_t n, pad[3]; uint8_t text[16]; } smhv_label_run;      /* 24 bytes; text beyond n is 0 */
typedef struct { smhv_firing firing; float mid[2], dir[2]; uint8_t rgba[4]; uint32_t n_runs; smhv_label_run run[6]; } smhv_label;   /* 216 bytes */
typedef struct { uint32_t n_labels, reserved; smhv_label label[SMHV_LABEL_MAX_EXTRA + SMHV_MAX_LINES]; } smhv_label_result;
/* A line without a label keeps its slot with n_runs = 0; slot order is extras first, then the detected lines; n_labels is the
 * number of slots (slots beyond it are zero). */
/* A glyph of the font: rows[0 .. 6], bit 4 = the leftmost column.  Host only.  SMHV_E_INVALID for a byte outside the 27. */
SMHV_API int smhv_label_font(uint8_t ch, uint8_t rows[7]);
/* Draws the labels onto the batch's render slab over frames [first, first + n), asynchronously on `stream`, behind whatever the
 * batch's previous render enqueued (a device-side wait), and writes the batch's label slab: one smhv_label_result per frame,
 * allocated by the first call.  ropt supplies the window and the viewport: out_w / out_h must be the most recent render's
 * (SMHV_E_STATE for another size or before the first render); hm (NULL: none) feeds the numbers whatever ropt->flags says.
 * SMHV_E_INVALID: what smhv_batch_render rejects in ropt, a wrong size, unknown flags, scale > 4, n_extra > SMHV_LABEL_MAX_EXTRA,
 * n_extra != 0 with extra == NULL, an rgba[3] != 255, n == 0 or a range beyond the batch's capacity.  A failed call enqueues
 * nothing.  The extras cross through pinned staging of the batch: a call with extras waits (host) until the previous call's copy
 * of them has run.  Works on a plain batch after smhv_batch_run and on a pipeline slot's batch after smhv_pipeline_wait, for both
 * searches.  The batch keeps a reference of hm as smhv_batch_render does. */
SMHV_API int smhv_batch_render_labels(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *ropt,
                                      const smhv_label_options *lopt, void *stream);
/* The batch's label slab: read is a synchronising host copy, ptr the device address (SMHV_E_STATE before the first
 * smhv_batch_render_labels): the strings and the placement without the pixels, for a caller that draws text itself. */
SMHV_API int smhv_batch_read_labels(smhv_batch *b, uint32_t first, uint32_t n, smhv_label_result *out);
SMHV_API int smhv_batch_labels_ptr(smhv_batch *b, void **d_labels);
/* The per-call path: exactly smhv_render_map_layers's image (smhv_render_map's with layers == NULL), then the labels; the image is
 * copied out once; *labels (optional) receives the slots.  With SMHV_LABEL_DETECTED the explicit `lines` are labelled
 * (SMHV_E_INVALID for more than SMHV_MAX_LINES).  Errors as smhv_render_map_layers and as above. */
SMHV_API int smhv_render_map_labeled(smhv_ctx *ctx, const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_render_layers *layers,
                                     const smhv_line *lines, uint32_t n_lines, const smhv_label_options *lopt, uint8_t *rgba,
                                     smhv_label_result *labels);

/* ---- map view: debug text and the vision debugger ---------------------------------------------------------------------------
 * What is left of the reference's window: the vision debugger (src/ui/debug.rs:350-475: RGB, HSV, Luma8, ocr_monochromaticy,
 * ocr_brightness and the three tests of debug_is_map_marker_color per fireteam, for the pixel under the cursor, printed in a small
 * window beside it), the text of the Debug menu's overlays (debug.rs:286-345: "{:.2}%\n{:?}" under every OCR box, "{}m" at every
 * scale bar, the red caption when a frame has no minimap rectangle).  The numbers come from k_probe, the picture is a pass of its
 * own over a finished image of the map view, as the labels are.  imgui's text and windows are not bit-reproducible: the library
 * pins ONE hard-edged restatement.  Every f32 operation is one operation, left to right, unfused.  W, H = out_w, out_h; sw, sh,
 * tx, ty = the render call's viewport (a scale of 0 means 1); S = smhv_debug_options.scale, 1 .. 4, 0 means 2, one value per call.
 * Font.  csrc/smh_font5x7_ascii.h: 97 glyphs in the label font's format and 6 x 9 cell -- the printable ASCII bytes 0x20 .. 0x7E,
 *   the degree sign 0xB0 and the plus-minus sign 0xB1; the label font's 27 glyphs have the same rows.  Drawn for this project.
 * Text runs.  A run = a position (x, y), rgba (alpha 255), flags, n <= SMHV_TEXT_MAX_BYTES text bytes; '\n' starts a new line at the
 *   run's x; a run has 1 + (number of '\n') lines, at most SMHV_TEXT_MAX_LINES (n == 0: one empty line).  The anchor P: with
 *   SMHV_TEXT_MAP_COORDS (x * sw + tx, y * sh + ty), otherwise (x, y) in window pixels.  Pixel (X, Y): cx = X + 0.5f, cy = Y + 0.5f;
 *   u = (cx - P.x) / (float)S, v = (cy - P.y) / (float)S; iu = floorf(u), iv = floorf(v).  Painted iff iu >= 0, iv >= 0, line = iv / 9 is
 *   less than the run's number of lines, iu / 6 is less than that line's number of characters, and the glyph of character iu / 6 of
 *   that line has its bit at column iu % 6 (< 5) and row iv % 9 - 1 (0 .. 6).  A run whose anchor is not finite paints nothing.
 *   Colour = the run's RGB, alpha 255.  The same list for every frame of a call.
 * Probe (debug.rs:357-385).  A window position (mx, my), the same for every frame of the call -> one smhv_probe per frame and
 *   position.  Every field is 0 (valid = 0) when the frame's map is closed or mx == FLT_MAX && my == FLT_MAX.  ix = (mx - tx) / sw,
 *   iy = (my - ty) / sh (MapViewport::inverse_xy); invalid if ix < 0 || iy < 0 (a NaN passes, as in the reference); px = ix as u32,
 *   py = iy as u32 (truncating, saturating, NaN -> 0); invalid if px >= w || py >= h (get_pixel_checked).  An invalid probe is all 0.
 *   rgb = the ui_map's pixel (px, py) as the batch or context holds it (after a grayscale run: the gray bytes).
 *   h, s, v = util/src/image.rs:159-187 in f32: r = R / 255.0f (g, b likewise); mx = max, mn = min, d = mx - mn; hue = 0 if mx == mn,
 *     else 60 * ((g - b) / d) if mx == r, else 60 * (((b - r) / d) + 2) if mx == g, else 60 * (((r - g) / d) + 4); hue < 0: hue + 360;
 *     h = hue as u16, s = ((100 * d) / mx) as u8 (NaN -> 0), v = (100 * mx) as u8 -- the operations of the marker predicate.
 *   luma = image 0.23.14's luma8: ((0.2126f * R + 0.7152f * G) + 0.0722f * B) as u8.  mono = the sum over all nine (a, b) of
 *     |p[a] - p[b]| (ocr_monochromaticy), brightness = the minimum channel (ocr_brightness).
 *   team_bits: bit 3 * team + k, team 0 = Alpha, 1 = Bravo, 2 = Charlie, (mh, ms, mv) that team's colour (smh_consts.h):
 *     k = 0: |mh - h| <= HUE_TOLERANCE; k = 1: s >= MIN_SAT && (|ms - s| <= SAT_TOLERANCE || |s - (ms - PLAYER_DIR_ARC_SAT)| <=
 *     SAT_TOLERANCE); k = 2: |mv - v| <= VIB_TOLERANCE.  "Some team has all three bits" is the predicate the pipeline runs.
 *   Text: smhv_probe_text writes the reference's string, eight lines joined by '\n': "RGB [r, g, b]", "HSV [h, s, v]", "Luma8 l",
 *     "OCRPixelSimilarity mono", "OCRBrightness brightness", "AlphaMarker [b0, b1, b2]", "BravoMarker [..]", "CharlieMarker [..]"
 *     with true / false for the bits.  The device builds the same bytes when it draws.
 * The debugger's picture (SMHV_DEBUG_DRAW_PROBES), for every valid probe, in list order.  C = the widest of the eight lines in
 *   characters; Wd = (float)(6 * S * C + 16), Hd = (float)(34 + 72 * S) (padding 8, swatch 10, 8, eight lines, 8).  THIS DEVIATES
 *   from the reference: the window is sized to its text in the place of imgui's wrapped 200 px window, and its background is
 *   opaque.  wp = (mx + 15.0f, my + 15.0f); if wp.x + Wd > (float)W || wp.y + Hd > (float)H then wp = ((mx - Wd) - 5.0f, (my - Hd) -
 *   5.0f) (debug.rs:415-420).  A fill of [a, b) paints pixel centres with a.x <= cx && cx < b.x && a.y <= cy && cy < b.y.  Painted in
 *   this order, later over earlier: (1) the fill [wp, (wp.x + Wd, wp.y + Hd)) in (15, 15, 15) (theme.rs:24, opaque); (2) the text
 *   as one run at (wp.x + 8.0f, wp.y + 26.0f) in (255, 255, 255); (3) the swatch, the fill [(wp.x + 8.0f, wp.y + 8.0f), ((wp.x + Wd) -
 *   8.0f, wp.y + 18.0f)) in rgb; (4) the pixel frame (debug.rs:444-463): pw = floorf(sw), ph = floorf(sh), ax = mx, ay = my; if pw > 1
 *   then ax = ax - fmodf(ax, pw); if ph > 1 then ay = ay - fmodf(ay, ph); corners (ax - pw, ay - ph) and (ax + ph, ay + ph) -- the
 *   reference's ph in both coordinates of the second corner is kept -- drawn by the SMHV_PRIM_RECT rule of "map view: layers" on
 *   these window coordinates, in (0, 0, 0) when ((float)r * 0.299f + (float)g * 0.587f) + (float)b * 0.114f > 186.0f, else (255, 255, 255).
 * The caption (SMHV_DEBUG_MINIMAP_CAPTION, debug.rs:335-343): a frame whose record has has_minimap == 0 (per call: the context's
 *   frame without a rectangle) gets "No minimap bounds detected or we don't need to detect them" in (255, 0, 0) as a window run at
 *   (10.0f, ((float)H - 10.0f) - (float)(9 * S)).
 * Paint order of the pass: the runs in list order, the caption, the probes; later over earlier, and everything over all that is
 *   already in the image -- THIS DEVIATES from the reference as the labels do: text always wins over strokes drawn before.  A frame
 *   whose map is closed gets nothing at all.  The reference's draw_fps (host wall times) and imgui's chrome are not drawn. */
#define SMHV_TEXT_MAX_RUNS 64u
#define SMHV_TEXT_MAX_BYTES 64u
#define SMHV_TEXT_MAX_LINES 8u
#define SMHV_TEXT_MAP_COORDS 1u       /* smhv_text_run.flags: (x, y) are map-ROI coordinates, through the viewport */
#define SMHV_MAX_PROBES 16u
#define SMHV_DEBUG_DRAW_PROBES 1u     /* smhv_debug_options.flags: the debugger's picture for every valid probe */
#define SMHV_DEBUG_MINIMAP_CAPTION 2u /*   ... the red caption on frames without a minimap rectangle */
typedef struct { float x, y; uint8_t rgba[4]; uint32_t flags; uint32_t n; uint8_t text[SMHV_TEXT_MAX_BYTES]; } smhv_text_run;   /* 84 bytes */
typedef struct { float x, y; } smhv_probe_point;                      /* window pixels */
typedef struct {
	uint32_t valid, px, py;
	uint8_t rgb[3], luma;
	uint16_t h; uint8_t s, v;
	uint16_t mono; uint8_t brightness, reserved0;
	uint32_t team_bits;                /* bit 3 * team + k */
	uint32_t reserved1;
} smhv_probe;                          /* 32 bytes */
typedef struct {
	uint32_t size;                     /* sizeof(smhv_debug_options) */
	uint32_t flags;                    /* SMHV_DEBUG_* */
	uint32_t scale;                    /* S: 1 .. 4, 0 = 2 */
	uint32_t n_runs;                   /* <= SMHV_TEXT_MAX_RUNS */
	const smhv_text_run *runs;         /* host memory; copied before the call returns; the same list for every frame of the call */
	uint32_t n_probes, reserved;       /* <= SMHV_MAX_PROBES */
	const smhv_probe_point *probes;    /* host memory, likewise */
} smhv_debug_options;
/* A glyph of the text font: rows[0 .. 6], bit 4 = the leftmost column.  Host only.  SMHV_E_INVALID for a byte outside the 97. */
SMHV_API int smhv_text_font(uint8_t ch, uint8_t rows[7]);
/* The debugger's string of a probe, NUL-terminated (at most 200 bytes with the NUL).  Host only.  SMHV_E_INVALID when cap is too small. */
SMHV_API int smhv_probe_text(const smhv_probe *p, char *out, size_t cap);
/* The numbers without any pixels: probes frames [first, first + n) at n_points <= SMHV_MAX_PROBES window positions through ropt's
 * viewport (nothing else of ropt is used but its size field), asynchronously on `stream`, into the batch's probe slab:
 * SMHV_MAX_PROBES smhv_probe per frame (allocated by the first call; entries beyond n_points are zeroed).  Needs a ui_map in the
 * batch (SMHV_E_STATE), no render.  SMHV_E_INVALID: null or wrongly sized ropt, n == 0 or a range beyond the capacity, n_points >
 * SMHV_MAX_PROBES, n_points != 0 with points == NULL.  The points cross through pinned staging of the batch under the rule the prims
 * follow.  A failed call enqueues nothing. */
SMHV_API int smhv_batch_probe(smhv_batch *b, uint32_t first, uint32_t n, const smhv_render_options *ropt, const smhv_probe_point *points,
                              uint32_t n_points, void *stream);
/* read: synchronising host copy of SMHV_MAX_PROBES * n entries; ptr: the device address (SMHV_E_STATE before the first probe) */
SMHV_API int smhv_batch_read_probes(smhv_batch *b, uint32_t first, uint32_t n, smhv_probe *out);
SMHV_API int smhv_batch_probes_ptr(smhv_batch *b, void **d_probes);
/* The pass over the batch's render slab, frames [first, first + n), asynchronously on `stream`, behind whatever the batch's
 * previous render, label or debug call enqueued; writes the probe slab too (dopt's probes).  ropt: the window (the most recent
 * render's: SMHV_E_STATE for another size or before the first render) and the viewport.  SMHV_E_INVALID: what smhv_batch_render
 * rejects in ropt (no heightmap is needed), a wrong size, unknown flags, scale > 4, n_runs > SMHV_TEXT_MAX_RUNS, n_probes >
 * SMHV_MAX_PROBES, a null list with a non-zero count, a run with n > SMHV_TEXT_MAX_BYTES, more than SMHV_TEXT_MAX_LINES lines, a byte
 * that has no glyph and is not '\n', rgba[3] != 255 or an unknown flag.  A failed call enqueues nothing.  Works on a plain batch and
 * on a pipeline slot's batch.  The first call that draws allocates the batch's item lists and string pool (about 12.5 KB per frame of
 * the batch's capacity); smhv_batch_probe allocates the probe slab alone. */
SMHV_API int smhv_batch_render_debug(smhv_batch *b, uint32_t first, uint32_t n, const smhv_render_options *ropt, const smhv_debug_options *dopt,
                                     void *stream);
/* The per-call path: exactly smhv_render_map_labeled's image (lopt == NULL: smhv_render_map_layers's, or smhv_render_map's with
 * layers == NULL too; `labels` is then not written), then this pass; one copy out.  probes (optional) receives SMHV_MAX_PROBES
 * entries.  With no runs, no probes and no flags the image is that call's, byte for byte.  Errors as those calls and as above. */
SMHV_API int smhv_render_map_debug(smhv_ctx *ctx, const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_render_layers *layers,
                                   const smhv_line *lines, uint32_t n_lines, const smhv_label_options *lopt, const smhv_debug_options *dopt,
                                   uint8_t *rgba, smhv_label_result *labels, smhv_probe *probes);

/* ---- remote-viewer feed: the web server's events of every processed frame ----------------------------------------------
 * The outward interface of a processed frame in the reference is the event stream of its web server (web/src/lib.rs:127-214),
 * fed once per new frame from src/ui/state.rs:81-88 and src/ui/map.rs:213-233: UpdateState, then Map -- but only when the CRC-32
 * (crc32fast::hash) of the map's bytes differs from the one the current texture was made from -- then Markers.  A feed is the
 * producer side of that protocol on the device: it hashes every frame's ui_map where it lies, applies the "changed since the
 * last texture" rule in frame order (the stored CRC lives in device memory and carries over from call to call) and writes the
 * byte-exact messages into one compact buffer, so what crosses to the host is proportional to what changed.  Transport
 * (sockets, HTTP) is the caller's.  The reference shows and sends debug_view.unwrap_or(map) (map.rs:210): with a debug view selected
 * that view is what is hashed and what goes out as the Map.  smhv_batch_feed_view / smhv_feed_frame_view take the view as
 * map_source; "the map" below is then that view, at its own width and height.
 * Messages, all little endian, each starting with its u16 id (the macro at lib.rs:74-126 numbers the variants from 1):
 *   UpdateState (state.rs:81-88, lib.rs:154-176): 03 00, f64 metres per pixel (0.0 for None: !has_mpx), then 01 and the record's
 *     minimap[4] = left, right, top, bottom as u32 when has_minimap, else 00.  27 or 11 bytes.
 *   Map (map.rs:213-226, lib.rs:130-140): 01 00, w and h as u32, then w*h*4 bytes of RGBA, tightly packed.  Sent iff the CRC-32 of
 *     those w*h*4 bytes differs from the stored CRC (nothing stored: sent); the stored CRC becomes this frame's when it is sent.
 *   Markers, custom = false (map.rs:228-233, lib.rs:142-152): 02 00, 00, n as u32, then per line x0, y0, x1, y1 as f32 (the
 *     record's lines, bit for bit).  Sent for every such frame, also with n = 0.
 * A frame whose map is closed, or whose status is not SMHV_FRAME_OK (the reference drops it on Err), sends nothing and leaves the
 * stored CRC alone (vision/mod.rs:282-288).  With SMHV_FEED_SNAPSHOT the call writes what a client that has just connected gets
 * for each of the given open frames instead (web/src/ws.rs:35-55), in that order: Map always, UpdateState only when the ratio or
 * the bounds are present, Markers only when there are lines; the stored CRC is neither used nor changed.
 * Buffer: one call's events replace the previous call's.  Frames are taken in index order, entries are in frame order and within
 * a frame in the order above.  The first message starts at offset 6 and every message at an offset = 6 (mod 16), so every Map
 * payload is 16-byte aligned; bytes between messages are unspecified.  A frame's events are written whole or not at all: a frame
 * fits when its last message ends at or before capacity_bytes; if the next frame does not fit the call stops there -- frames_done
 * says how many frames of [first, first + n) were consumed (frames without events that follow the last fitting frame included),
 * the stored CRC reflects only those, and the caller continues with first + frames_done.  A feed is used by one thread at a time. */
#define SMHV_WEB_MAP 1u
#define SMHV_WEB_MARKERS 2u
#define SMHV_WEB_UPDATE_STATE 3u
#define SMHV_WEB_HEIGHTMAP 4u
#define SMHV_WEB_FIT_TO_MINIMAP 5u
#define SMHV_FEED_SNAPSHOT 1u   /* ws.rs:35-55 for the given frames: Map always, UpdateState / Markers only when they carry
                                   something; the feed's stored CRC is neither used nor changed */
typedef struct smhv_feed smhv_feed;
typedef struct { uint64_t offset; uint32_t length, frame, kind, crc; } smhv_feed_entry;   /* a message: bytes [offset, offset + length) of the buffer,
                                   frame = its index in the batch, kind = SMHV_WEB_*, crc = CRC-32 of the Map payload of that frame for
                                   the call's source (the ui_map, or the debug view given as map_source) */
typedef struct { uint32_t n_entries, frames_done, n_maps, has_last_crc, last_crc, reserved; uint64_t bytes_used; } smhv_feed_header;   /* bytes_used: the end
                                   of the last message; has_last_crc / last_crc: the stored CRC after the call */
/* capacity_bytes: the message buffer; max_frames: the most frames one call covers (1 .. 65535) */
SMHV_API int smhv_feed_create(smhv_ctx *ctx, uint64_t capacity_bytes, uint32_t max_frames, smhv_feed **out);
SMHV_API void smhv_feed_destroy(smhv_feed *feed);
/* forget the stored CRC: the next open frame sends its map.  Waits (host) for the feed's previous call. */
SMHV_API int smhv_feed_reset(smhv_feed *feed);
/* The events of frames [first, first + n) of the batch, drawn from its ui slab and records as they are when `stream` reaches the
 * call (as smhv_batch_render: a plain batch after smhv_batch_run, or a pipeline slot's batch after smhv_pipeline_wait, on either
 * search schedule).  Asynchronous: three kernels on `stream` (CRC, plan, compacting copy) and no host round trip; the library
 * orders the call behind the feed's previous call, on whatever stream that was.  SMHV_E_INVALID: capacity_bytes below one
 * frame's worst case for this batch's geometry (6 + 32 + (10 + w*h*4 rounded up to 16) + 519), n == 0, a range beyond the batch's
 * capacity or beyond the feed's max_frames, unknown flags, a batch on another device; SMHV_E_STATE: no run of the batch has
 * produced a ui_map.  A failed call enqueues nothing. */
SMHV_API int smhv_batch_feed(smhv_batch *b, smhv_feed *feed, uint32_t first, uint32_t n, uint32_t flags, void *stream);
/* The same with a debug view as the Map (map.rs:210).  map_source = SMHV_VIEW_NONE is smhv_batch_feed, byte for byte; otherwise one
 * of the five SMHV_VIEW_*: the Map message is 01 00, the VIEW's width and height as u32 and its RGBA bytes -- exactly the bytes
 * "Map sources" under "map view: layers" pins for a batch ((L, L, L, 255) from the ocr, scales or mask plane; the colour ui_map with
 * every non-marker pixel (0, 0, 0, 255); the colour ui_map's bottom right quarter, alpha 255), generated from the slabs where they
 * lie: nothing the size of a batch is materialised.  The "changed since the last texture" rule runs over those bytes.  A feed has ONE
 * stored CRC whatever the source, as the reference has one texture CRC: a call with another source compares against it, so
 * switching the source normally sends a Map and switching back sends one again.  UpdateState, Markers, closed and non-OK frames,
 * SMHV_FEED_SNAPSHOT, the layout, the capacity cut, frames_done and the chaining are unchanged.  SMHV_E_INVALID: an unknown
 * map_source, or capacity_bytes below one frame's worst case computed with the SOURCE's width and height (brq_w x brq_h = w/2 x h/2
 * for the OCR input, the scales input and the cropped quarter); SMHV_E_STATE: smhv_batch_render_layers' conditions for the source.
 * A failed call enqueues nothing and changes nothing. */
SMHV_API int smhv_batch_feed_view(smhv_batch *b, smhv_feed *feed, uint32_t first, uint32_t n, uint32_t flags, uint32_t map_source, void *stream);
/* Waits for the feed's last call and copies the header, then n_entries entries (entries may be NULL) and bytes_used bytes (bytes
 * may be NULL) -- nothing else crosses.  SMHV_E_INVALID when max_entries or cap is too small (the header is filled in then). */
SMHV_API int smhv_feed_read(smhv_feed *feed, smhv_feed_header *header, smhv_feed_entry *entries, uint32_t max_entries, uint8_t *bytes, uint64_t cap);
/* device addresses of the header, the entries (3 * max_frames) and the message buffer (valid for the life of the feed) */
SMHV_API int smhv_feed_ptrs(smhv_feed *feed, void **d_header, void **d_entries, void **d_bytes);
/* The per-call path: the context's current frame -- the ui_map smhv_crop_to_map left on the device -- with explicit lines
 * (n_lines <= SMHV_MAX_LINES; custom markers travel in a message of their own: smhv_web_event_markers), mpx (NULL: None) and
 * minimap = {left, right, top, bottom} (NULL: None), as frame 0.  On the context's stream; SMHV_E_INVALID before load_frame /
 * crop_to_map, SMHV_E_STATE when the map is closed. */
SMHV_API int smhv_feed_frame(smhv_ctx *ctx, smhv_feed *feed, const smhv_line *lines, uint32_t n_lines, const double *mpx, const uint32_t minimap[4],
                             uint32_t flags);
/* The same with a debug view as the Map: the payload is exactly what smhv_get_debug_view(ctx, map_source, ...) returns at that
 * moment (the view is drawn into device memory of the feed and hashed there); SMHV_VIEW_NONE is smhv_feed_frame.  Errors as
 * smhv_feed_frame, the capacity measured with the view's size; SMHV_E_INVALID for an unknown map_source. */
SMHV_API int smhv_feed_frame_view(smhv_ctx *ctx, smhv_feed *feed, const smhv_line *lines, uint32_t n_lines, const double *mpx, const uint32_t minimap[4],
                                  uint32_t flags, uint32_t map_source);
/* ---- remote-viewer feed: map tiles ------------------------------------------------------------------------------------------
 * A Map is the whole picture and is sent whenever one pixel differs.  smhv_batch_feed_tiles / smhv_feed_frame_tiles are
 * smhv_batch_feed / smhv_feed_frame with one more message, MapTiles, that carries only the tiles of the map that changed.  THE
 * REFERENCE HAS NO SUCH MESSAGE (its web server sends Maps only): a client that turns tiles on must know id 6; the calls without
 * tiles are unchanged and never send it.  The rule, for host and device, stands once in csrc/smh_maptiles.h.
 * Tile grid: a map of w x h pixels is cut into tiles of 64 x 16 pixels counted from its pixel (0, 0): tiles_x = ceil(w / 64),
 * tiles_y = ceil(h / 16), tile index t = ty * tiles_x + tx; tiles of the last column and row are clipped, cw = min(64, w - 64 tx),
 * ch = min(16, h - 16 ty).  A tile's bytes are its ch rows of cw RGBA pixels, tightly packed, then zero bytes up to the next
 * multiple of 16.
 * MapTiles, all fields little endian:
 *    0  u16  06 00                                  14  u32  n, the number of tiles
 *    2  u32  w                                      18  u32  base_crc: the CRC-32 of the map these tiles are applied to
 *    6  u32  h                                      22  u32  crc: the CRC-32 of the map after they are applied
 *   10  u16  64                                     26  n x u32 tile indices, strictly ascending, then zero bytes up to a multiple of 16
 *   12  u16  16                                     26 + pad16(4 n)  the n tiles in that order, each padded as above
 * Messages start at offsets = 6 (mod 16) as before, so the index list and every tile start on a 16-byte boundary.  Length
 * L = 26 + pad16(4 n) + the sum of pad16(4 cw ch) over the tiles.  A tile is in the list iff any of its bytes differs from the same
 * bytes of the base map; alpha counts.
 * What a frame sends: an open SMHV_FRAME_OK frame sends UpdateState and Markers exactly as before, and between them nothing when its
 * CRC equals the texture's CRC as the frame finds it (the rule above, unchanged: equal CRCs count as equal maps), MapTiles against
 * its base when it has a base and L < 10 + 4 w h, otherwise the Map, byte for byte the message above.  The base of a frame is the map
 * of the nearest earlier open OK frame of the same call; the base of the first such frame of a call is the feed's KEPT MAP, usable
 * iff the feed has a stored CRC, that CRC equals the kept map's CRC, and the kept map's w, h equal this call's.  After a call the kept
 * map is the map of the last CONSUMED open OK frame (a call that consumed none leaves it unchanged); the stored CRC moves exactly as
 * before.  Hence: smhv_feed_reset leads to a Map; a call without tiles that sent a Map makes the kept map stale, so the next tile
 * call sends a Map, and one that sent none leaves it usable; a capacity cut keeps the map of the frame where the call stopped;
 * another map size leads to a Map.  Every tile changed always gives L > 10 + 4 w h, so a wholly new picture goes out as a Map and
 * one frame's worst case in the buffer is the one above.  Entries: kind = 6, length = L, crc = the frame's CRC.  The header is
 * unchanged: n_maps counts Map messages only.
 * flags must be 0: SMHV_FEED_SNAPSHOT is SMHV_E_INVALID (a snapshot has no base).  The source is the ui_map only; a debug view as the
 * Map is out of scope here (no map_source).  Every other check, its order and its text are smhv_batch_feed's / smhv_feed_frame's; a
 * failed call enqueues nothing, changes nothing and allocates nothing.  Tile calls and calls without tiles may alternate on one feed
 * and chain as before.  The kept map and the per-frame tile bitmaps are device memory of the feed, made by the first tile call and
 * freed by smhv_feed_destroy.  No host round trip inside a call. */
#define SMHV_WEB_MAP_TILES 6u
SMHV_API int smhv_batch_feed_tiles(smhv_batch *b, smhv_feed *feed, uint32_t first, uint32_t n, uint32_t flags, void *stream);
SMHV_API int smhv_feed_frame_tiles(smhv_ctx *ctx, smhv_feed *feed, const smhv_line *lines, uint32_t n_lines, const double *mpx, const uint32_t minimap[4],
                                   uint32_t flags);
/* The rest of the protocol, host only (no device needed).  Encoders: *len <- the message's length; the message is written when
 * out != NULL and cap >= *len (out == NULL asks for the length), SMHV_E_INVALID when cap is too small.
 *   Markers (lib.rs:142-152): 02 00, custom as a byte, n as u32, n x 4 f32.
 *   Heightmap (lib.rs:178-206): 04 00 01 00 -- the flag, then a pad byte that keeps the texels on an even offset -- w, h as u32,
 *     bounds[0] and bounds[1] (the reference's bounds[0][0], bounds[0][1]) as i32, scale[2] as f32, then w*h u16 texels: 24 bytes
 *     and the texels; data == NULL is None: 04 00 00.
 *   HeightmapFitToMinimap (lib.rs:208-213): 05 00 and the flag as a byte.
 * Interaction::deserialize (lib.rs:37-71), the client's replies: *kind <- 1 (AddCustomMarker: exactly 16 more bytes, line <- p0.x,
 * p0.y, p1.x, p1.y bit for bit) or 2 (DeleteCustomMarker: exactly 4 more bytes, *index), or 0 for anything else (None). */
SMHV_API int smhv_web_event_markers(const smhv_line *lines, uint32_t n, int custom, uint8_t *out, uint64_t cap, uint64_t *len);
SMHV_API int smhv_web_event_heightmap(const uint16_t *data, uint32_t w, uint32_t h, const int32_t bounds[4], const float scale[3], uint8_t *out,
                                      uint64_t cap, uint64_t *len);
SMHV_API int smhv_web_event_fit(int fit_to_minimap, uint8_t *out, uint64_t cap, uint64_t *len);
SMHV_API int smhv_web_interaction_parse(const uint8_t *data, uint64_t len, uint32_t *kind, float line[4], uint32_t *index);

/* ---- reach map: the firing solution from an origin to every window pixel -----------------------------------------------------
 * Where a tube at an origin can reach, and in which band of elevation: the firing solution of "firing solutions" evaluated for
 * every pixel of a map view's window.  The reference draws no such picture; the arithmetic is the reference's alone (markers.rs,
 * squadex::milliradians::calc), restated for a dense pass.  Every f32 / f64 operation is one operation, left to right, unfused.
 * Target.  Frame f, window pixel (X, Y): cx = X + 0.5f, cy = Y + 0.5f; sw, sh, tx, ty = the render options' viewport_scale (0 = 1)
 *   and viewport_top_left.  t = ((cx - tx) / sw, (cy - ty) / sh) in f32 (MapViewport::inverse_xy), map-ROI coordinates.
 * The pixel's value is a function of the firing solution of the line (o, t), direction 0, by the rule "firing solutions" pins for an
 *   explicit line: P0 = o * s + t_, P1 = t * s + t_ (translate_xy, f32); the heightmap branch when the frame has a minimap rectangle,
 *   a heightmap is given and all four rounded coordinates lie inside it (range = sqrt(dx*dx + dy*dy) of the heightmap coordinates,
 *   alt = height(P1) - height(P0)); else the scales branch with alt = 0 when the frame has m/px, meters =
 *   sqrt(ax*ax + ay*ay) * mpx with ax = (double)o.x - (double)t.x, ay likewise (Marker::new, the labels' rule for a line that is
 *   not a detected one); else none.  SMHV_RENDER_BOUNDS_OFFSET acts as SMHV_FIRING_BOUNDS_OFFSET.  The heightmap passed to the call
 *   feeds the numbers whatever ropt->flags says.
 * Origin o (smhv_reach_options.origin_mode).  SMHV_REACH_ORIGIN_POINT: origin[2], map-ROI coordinates, the same for every frame.
 *   SMHV_REACH_ORIGIN_LINE_P0 / _LINE_P1: that end of rec.lines[line] of each frame, read on the device.  A frame with
 *   n_lines <= line, a closed map or an origin that is not finite has NO origin: class 0 everywhere, a result of zeros.  The
 *   per-call path takes POINT only and has no closed map (it is stateless: it takes what it is given).
 * Class byte.  No atan is evaluated: in-range-ness and the mil band are decided in exact IEEE arithmetic.  m = meters, V^2, V^4, g
 *   the constants of "firing solutions" (V^2 = pow(109.890938, 2), V^4 = pow(109.890938, 4), g = 9.8):
 *     0        nothing: no origin, source NONE, a coordinate of t not finite, or m NaN.
 *     1        out of range: disc = V^4 - g * (g * (m * m) + 2.0 * alt * V^2) is < 0 (or NaN) -- exactly "mils[0] is NaN".
 *     2 + k    in range, k = 0 .. 7: q = (V^2 + sqrt(disc)) / (g * m); k = the number of j in 0 .. 6 with q >= T_j, T_j =
 *              tan(mils_j * pi / 3200) for mils_j = 900, 1000, ..., 1500, as the f64 constants smhv_reach_thresholds returns
 *              (0x1.37efd8d87607ep+0, 0x1.7f218e25a745fp+0, 0x1.def13b73c1408p+0, 0x1.3504f333f9de6p+1, 0x1.a5f59e90600d8p+1,
 *              0x1.41bfee2424769p+2, 0x1.44e6c595afdc2p+3).  Band k holds the elevations of [800 + 100 k, 900 + 100 k) mils, band 0
 *              everything below 900, band 7 everything from 1500 up; m == 0 gives q = +inf and k = 7.
 *     | 0x80   a range ring, only when ring_m > 0 and the class is not 0: set iff floor(m / ring_m) of this pixel differs from that
 *              of pixel (X + 1, Y) or of pixel (X, Y + 1), each evaluated by the same rule even where it lies outside the window.  A
 *              neighbour whose source differs from this pixel's, or whose class would be 0, does not count.
 * Paint (SMHV_REACH_PAINT), into the batch's render slab, over whatever is there.  p = the palette entry of the class
 *   (out_of_range for 1, band[k] for 2 + k), a = its fourth byte: each of R, G, B becomes (c * (255 - a) + p * a + 127) / 255 in
 *   integers; on a ring pixel the same blend with ring[4] follows.  The image's alpha byte is untouched; class 0 leaves the pixel
 *   as it is.  THIS DEVIATES from the reference's layering as the labels do: the tint lies over everything already drawn, the
 *   marker strokes included.  A caller draws the text passes (labels, debug text) afterwards.
 * Classes (SMHV_REACH_CLASSES): the class bytes, out_w * out_h per frame, rows and frames tightly packed, the call's first frame
 *   at d_classes, into caller-provided device memory.  Needs no render slab.
 * Summary.  One smhv_reach_result per frame in the batch's reach slab (allocated by the first call): valid = 1 iff the frame had an
 *   origin (else every field is 0); origin = o; count[c - 1] = window pixels of class c (ring bit ignored), c = 1 .. 9; ring =
 *   window pixels with the ring bit; source_mask: bit 1 << s iff some window pixel has a class other than 0 and source s
 *   (SMHV_FIRING_SCALES, _HEIGHTMAP), bit 0 iff some window pixel has class 0. */
#define SMHV_REACH_PAINT 1u            /* smhv_reach_options.flags: tint the render slab (per call: implied by rgba_inout) */
#define SMHV_REACH_CLASSES 2u          /*   ... write the class bytes (per call: implied by classes) */
#define SMHV_REACH_ORIGIN_POINT 0u     /* smhv_reach_options.origin_mode */
#define SMHV_REACH_ORIGIN_LINE_P0 1u
#define SMHV_REACH_ORIGIN_LINE_P1 2u
#define SMHV_REACH_OUT_OF_RANGE 1u     /* the class byte */
#define SMHV_REACH_BAND0 2u
#define SMHV_REACH_RING 0x80u
typedef struct {
	uint32_t size;                       /*  0: sizeof(smhv_reach_options) == 80 */
	uint32_t flags;                      /*  4: SMHV_REACH_PAINT | SMHV_REACH_CLASSES (0: the summary alone) */
	uint32_t origin_mode;                /*  8: SMHV_REACH_ORIGIN_* */
	uint32_t line;                       /* 12: _LINE_P0 / _LINE_P1: which line of the record, < SMHV_MAX_LINES */
	float origin[2];                     /* 16: _POINT: the origin, map-ROI coordinates */
	double ring_m;                       /* 24: metres between range rings; 0 = none; finite, >= 0 */
	uint8_t out_of_range[4];             /* 32: the palette: R, G, B and the blend weight a */
	uint8_t band[8][4];                  /* 36 */
	uint8_t ring[4];                     /* 68 */
	uint32_t reserved[2];                /* 72 */
} smhv_reach_options;
typedef struct {
	uint32_t valid;                      /*  0 */
	uint32_t source_mask;                /*  4 */
	float origin[2];                     /*  8 */
	uint32_t count[9];                   /* 16: classes 1 .. 9 */
	uint32_t ring;                       /* 52 */
	uint32_t reserved[2];                /* 56 */
} smhv_reach_result;                     /* 64 bytes */
/* Host only.  Fills *opt: size, flags = PAINT, origin_mode = POINT at (0, 0), ring_m = 0 and the palette -- out of range
 * (200, 30, 30, 96); the bands from flat fire to high angle (40, 90, 255), (0, 170, 255), (0, 220, 200), (0, 230, 110), (120, 235, 0),
 * (220, 230, 0), (255, 180, 0), (255, 120, 40), each with a = 72; ring (255, 255, 255, 160). */
SMHV_API int smhv_reach_defaults(smhv_reach_options *opt);
/* Host only.  The seven T_j above. */
SMHV_API int smhv_reach_thresholds(double out[7]);
/* The reach map of frames [first, first + n), asynchronously on `stream`; the frames' results in the reach slab are cleared on the
 * stream ahead of the kernel.  ropt supplies the window and the viewport (quad, background and the HEIGHTMAP / MARKERS flags are
 * not used); hm (NULL: none) feeds the numbers.  With PAINT the call runs behind whatever the batch's previous render enqueued and
 * ropt->out_w / out_h must be the most recent render's (SMHV_E_STATE for another size or before the first render).  Without PAINT
 * only the records are read: a plain batch after smhv_batch_run, or a pipeline slot's batch after smhv_pipeline_wait, for both
 * searches (a batch that has not run has closed maps only).  SMHV_E_INVALID: what smhv_batch_render rejects in ropt, a wrong size,
 * unknown flags, an unknown origin_mode, line >= SMHV_MAX_LINES, a ring_m that is negative or not finite, CLASSES with
 * d_classes == NULL, n == 0, a range beyond the batch's capacity, a heightmap on another device.  A failed call enqueues nothing.
 * The batch keeps a reference of hm as smhv_batch_render does. */
SMHV_API int smhv_batch_reach(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *ropt,
                              const smhv_reach_options *opt, void *d_classes, void *stream);
/* The batch's reach slab: read is a synchronising host copy, ptr the device address (SMHV_E_STATE before the first smhv_batch_reach) */
SMHV_API int smhv_batch_read_reach(smhv_batch *b, uint32_t first, uint32_t n, smhv_reach_result *out);
SMHV_API int smhv_batch_reach_ptr(smhv_batch *b, void **d_reach);
/* The per-call path, stateless like smhv_firing_solutions: mpx (NULL: none), minimap = {left, right, top, bottom} (NULL: none), hm
 * (NULL: none); origin_mode must be POINT.  rgba_inout (host, out_w * out_h * 4 bytes, an image of any smhv_render_map* call or any
 * other) is tinted in place; classes (host, out_w * out_h bytes) receives the class bytes; either may be NULL, not both; result
 * (optional) receives the summary.  opt->flags is checked for unknown bits and otherwise not used.  Runs on the context's stream. */
SMHV_API int smhv_reach_map(smhv_ctx *ctx, const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_reach_options *opt, const double *mpx,
                            const uint32_t minimap[4], uint8_t *rgba_inout, uint8_t *classes, smhv_reach_result *result);

/* ---- terrain clearance: does a shell's arc clear the heightmap on its way ----------------------------------------------------
 * The firing solutions and the reach map read the heightmap at the two end points only.  This pass looks at what lies between them:
 * it samples the heightmap along the line and holds the high-angle arc (the one mortar_mils' elevation belongs to) and the straight
 * sight line against the terrain.  The reference computes no such thing; the arithmetic is "firing solutions"' alone.  Every
 * operation is one IEEE f64 operation, left to right, unfused; V^2, V^4, g are the constants of "firing solutions".
 * A verdict exists only on the heightmap branch of "firing solutions": a minimap rectangle, a heightmap, and all four rounded end-point
 *   coordinates inside it.  Everything else (the scales branch too: it has no terrain) is status NONE, a record of zeros.
 * The rule, direction 0 (firing from P0 at P1), with that branch's own values: (x0, y0), (x1, y1) = the heightmap coordinates in f64,
 *   W x H the heightmap, d = sqrt(dx*dx + dy*dy), h0 = height(P0), h1 = height(P1), alt = h1 - h0, S = opt->samples:
 *   1. disc = V^4 - g * (g * (d * d) + 2.0 * alt * V^2).  !(disc >= 0): OUT_OF_RANGE.  d == 0.0: CLEAR with no samples (zero counts,
 *      first_blocked = S, min_margin = 0, min_at = 0).
 *   2. q = (V^2 + sqrt(disc)) / (g * d), the tangent of the high angle.
 *   3. For each interior sample k = 1 .. S - 1, t = (double)k / (double)S:
 *        texel   sx = x0 + (x1 - x0) * t, sy = y0 + (y1 - y0) * t, each rounded half away from zero `as i32` and then clamped into
 *                [0, W - 1] and [0, H - 1]; v = the texel there.  (Each axis depends on its own end coordinates and k alone.)
 *        terrain z = ((double)v / 65535.0) * zscale - h0, zscale = (double)scale[2] / 0.1953125: metres over the origin.
 *        arc     x = d * t; a = x * q - ((g * (x * x)) * (1.0 + q * q)) / (2.0 * V^2).
 *        margin  m = a - z.  The sample blocks the arc iff m < opt->margin_m.
 *        sight   l = alt * t.  The sample blocks the line of sight iff l < z.
 *   4. BLOCKED iff some sample blocks the arc, else CLEAR.  first_blocked = the least blocking k (S: none), n_blocked = how many
 *      block the arc, los_blocked = how many block the sight line.  min_margin = the least m, min_at its k: best starts at +inf and
 *      is replaced only when m < best, so a NaN never wins and ties go to the lowest k; min_at is 0 while nothing has replaced it, and
 *      min_margin is reported as 0 when S == 1.
 *   An OUT_OF_RANGE line has no arc: first_blocked = S, n_blocked = 0, min_margin = 0, min_at = 0; its los_blocked is counted as above.
 *   Direction 1 is the same rule on the line (P1, P0): end coordinates swapped, h0 := h1, alt := -alt.
 * Profile (optional), direction 0: SMHV_CLEAR_MAX_SAMPLES + 1 floats per line, entry k = 0 .. S is (float)(((double)v / 65535.0) *
 *   zscale) at sample k's texel -- entries 0 and S at the end points' own rounded texels -- and the entries past S are 0.  A line
 *   without a verdict (NONE), or beyond the record's n_lines, is all zeros.  A frame is SMHV_MAX_LINES such rows.
 * Dense (the clearance map): origin and target per window pixel are exactly the reach map's -- origin_mode, line, origin, the "no
 *   origin" rule, the viewport and the heightmap coordinates of "reach map" -- and the rule above, direction 0, gives one byte per
 *   pixel: the status, | SMHV_CLEAR_LOS_BLOCKED wherever the status is not NONE and some sample blocks the sight line (out-of-range
 *   pixels included).  Paint (SMHV_CLEAR_PAINT) goes over the render slab by the reach map's integer blend: the palette entry of the
 *   status (out_of_range, clear, blocked), then on a pixel with the LOS bit los[4]; a weight of 0 leaves the pixel as it is.  Bytes
 *   (SMHV_CLEAR_BYTES): out_w * out_h per frame, tightly packed, into caller memory.  Summary: one smhv_clearance_map_result per
 *   frame, cleared on the stream ahead of the kernel: valid = 1 iff the frame had an origin (else zeros), origin, count[s - 1] =
 *   window pixels of status s = 1 .. 3, los_blocked = window pixels with the LOS bit. */
#define SMHV_CLEAR_MAX_SAMPLES 256u
#define SMHV_CLEAR_PAINT 1u            /* smhv_clearance_options.flags: tint the render slab (the map; per call: implied by rgba_inout) */
#define SMHV_CLEAR_BYTES 2u            /*   ... write the status bytes (the map; per call: implied by bytes) */
#define SMHV_CLEAR_NONE 0u             /* status */
#define SMHV_CLEAR_OUT_OF_RANGE 1u
#define SMHV_CLEAR_CLEAR 2u
#define SMHV_CLEAR_BLOCKED 3u
#define SMHV_CLEAR_LOS_BLOCKED 0x80u   /* the map's byte: | this */
typedef struct {
	uint32_t size;                       /*  0: sizeof(smhv_clearance_options) == 64 */
	uint32_t flags;                      /*  4: SMHV_CLEAR_PAINT | SMHV_CLEAR_BYTES (the map only; 0: the summary alone) */
	uint32_t samples;                    /*  8: S, 1 .. SMHV_CLEAR_MAX_SAMPLES */
	uint32_t origin_mode;                /* 12: the map: SMHV_REACH_ORIGIN_* */
	uint32_t line;                       /* 16: the map, _LINE_P0 / _LINE_P1: which line of the record, < SMHV_MAX_LINES */
	uint32_t reserved0;                  /* 20 */
	float origin[2];                     /* 24: the map, _POINT: the origin, map-ROI coordinates */
	double margin_m;                     /* 32: metres the arc must keep over the terrain; finite, >= 0 */
	uint8_t out_of_range[4];             /* 40: the palette: R, G, B and the blend weight a */
	uint8_t clear[4];                    /* 44 */
	uint8_t blocked[4];                  /* 48 */
	uint8_t los[4];                      /* 52 */
	uint32_t reserved[2];                /* 56 */
} smhv_clearance_options;
typedef struct {
	uint32_t status;                     /*  0: SMHV_CLEAR_NONE / _OUT_OF_RANGE / _CLEAR / _BLOCKED */
	uint32_t first_blocked;              /*  4: the least k that blocks the arc; S when there is none */
	uint32_t n_blocked;                  /*  8 */
	uint32_t los_blocked;                /* 12: samples that block the sight line (a count) */
	double min_margin;                   /* 16 */
	uint32_t min_at;                     /* 24 */
	uint32_t reserved;                   /* 28 */
} smhv_clearance_dir;                    /* 32 bytes */
typedef struct { smhv_clearance_dir dir[2]; } smhv_clearance;   /* 64 bytes: [0] from p0 at p1, [1] from p1 at p0 */
typedef struct {
	uint32_t n_lines, reserved;          /* == the record's n_lines; lines beyond it are zero */
	smhv_clearance line[SMHV_MAX_LINES];
} smhv_clearance_result;
typedef struct {
	uint32_t valid;                      /*  0 */
	uint32_t reserved;                   /*  4 */
	float origin[2];                     /*  8 */
	uint32_t count[3];                   /* 16: statuses 1 .. 3 */
	uint32_t los_blocked;                /* 28 */
} smhv_clearance_map_result;             /* 32 bytes */
/* Host only.  Fills *opt: size, flags = PAINT, samples = 64, origin_mode = POINT at (0, 0), margin_m = 0 and the palette --
 * out_of_range and clear (0, 0, 0, 0), blocked (230, 40, 40, 110), los (0, 0, 0, 70). */
SMHV_API int smhv_clearance_defaults(smhv_clearance_options *opt);
/* The clearance of the detected lines of frames [first, first + n), asynchronously on `stream`, from the batch's records (n_lines,
 * the lines, the minimap rectangle): a plain batch after smhv_batch_run, or a pipeline slot's batch after smhv_pipeline_wait, for
 * both searches.  hm (NULL: none -- NONE everywhere), fopt (NULL: defaults) as smhv_firing_solutions takes them; of opt, samples and
 * margin_m apply (flags are checked).  d_profiles (device memory, NULL: none): n * SMHV_MAX_LINES * (SMHV_CLEAR_MAX_SAMPLES + 1)
 * floats, the call's first frame first.  The results go to the batch's clearance slab (allocated by the first call).
 * SMHV_E_INVALID: a wrong size, unknown flags, samples 0 or above SMHV_CLEAR_MAX_SAMPLES, a margin_m that is negative or not finite,
 * what smhv_firing_solutions rejects in fopt, n == 0, a range beyond the batch's capacity, a heightmap on another device.  A failed
 * call enqueues nothing.  The batch keeps a reference of hm as smhv_batch_render does. */
SMHV_API int smhv_batch_clearance(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_firing_options *fopt,
                                  const smhv_clearance_options *opt, void *d_profiles, void *stream);
/* The batch's clearance slab: read is a synchronising host copy, ptr the device address (SMHV_E_STATE before the first
 * smhv_batch_clearance) */
SMHV_API int smhv_batch_read_clearance(smhv_batch *b, uint32_t first, uint32_t n, smhv_clearance_result *out);
SMHV_API int smhv_batch_clearance_ptr(smhv_batch *b, void **d_clearance);
/* The same for explicit lines, stateless like smhv_firing_solutions: n lines in map-ROI coordinates, minimap = {left, right, top,
 * bottom} (NULL: none), hm (NULL: none), fopt (NULL: defaults).  out receives n records; profiles (host, NULL: none) n *
 * (SMHV_CLEAR_MAX_SAMPLES + 1) floats.  Runs on the context's stream. */
SMHV_API int smhv_clearance_lines(smhv_ctx *ctx, const smhv_line *lines, uint32_t n, const uint32_t minimap[4], const smhv_heightmap *hm,
                                  const smhv_firing_options *fopt, const smhv_clearance_options *opt, smhv_clearance *out, float *profiles);
/* The clearance map of frames [first, first + n), asynchronously on `stream`; everything smhv_batch_reach says about ropt, hm, PAINT
 * (behind the batch's previous render, the most recent render's window), the records and its errors holds here, with
 * smhv_clearance_options in place of smhv_reach_options (its errors as smhv_batch_clearance lists them, an unknown origin_mode and
 * line >= SMHV_MAX_LINES besides) and SMHV_CLEAR_BYTES with d_bytes == NULL refused.  The summaries go to the batch's clearance-map
 * slab (allocated by the first call). */
SMHV_API int smhv_batch_clearance_map(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *ropt,
                                      const smhv_clearance_options *opt, void *d_bytes, void *stream);
SMHV_API int smhv_batch_read_clearance_map(smhv_batch *b, uint32_t first, uint32_t n, smhv_clearance_map_result *out);
SMHV_API int smhv_batch_clearance_map_ptr(smhv_batch *b, void **d_clearance_map);
/* The per-call path, stateless like smhv_reach_map: minimap = {left, right, top, bottom} (NULL: none), hm (NULL: none); origin_mode
 * must be POINT.  rgba_inout (host, out_w * out_h * 4 bytes) is tinted in place; bytes (host, out_w * out_h) receives the status
 * bytes; either may be NULL, not both; result (optional) receives the summary.  opt->flags is checked for unknown bits and
 * otherwise not used.  Runs on the context's stream. */
SMHV_API int smhv_clearance_map(smhv_ctx *ctx, const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_clearance_options *opt,
                                const uint32_t minimap[4], uint8_t *rgba_inout, uint8_t *bytes, smhv_clearance_map_result *result);

/* ---- terrain relief: contour lines, hillshade and heights of every window pixel ------------------------------------------------
 * The reach map says where a tube can reach and the clearance map where the arc is blocked; this pass shows why: the shape of the
 * ground under a map view's window -- the terrain height of every pixel, a hillshade value and whether a contour line or an index
 * contour passes there.  The reference draws no such picture; the coordinates are "firing solutions"' alone.  Every operation is one
 * IEEE f64 operation, left to right, unfused (a product is rounded before it is added; (double) of an integer or an f32 is exact),
 * but for the rectangle, which stays f32 as the firing solutions have it.  W x H = the heightmap, texel (i, j) = data[j * W + i].
 * Pixel.  Frame f, window pixel (X, Y): cx = X + 0.5f, cy = Y + 0.5f in f32.  R = {l, t, r, b} = the heightmap's rectangle of "firing
 *   solutions" in f32, from the frame's minimap rectangle through the render options' viewport (viewport_scale, 0 = 1;
 *   viewport_top_left); SMHV_RENDER_BOUNDS_OFFSET acts as SMHV_FIRING_BOUNDS_OFFSET.  rw = (double)(r - l), rh = (double)(b - t), the
 *   differences in f32.  px = (((double)cx - (double)l) / rw) * (double)W, py = (((double)cy - (double)t) / rh) * (double)H.  The
 *   window position itself is the translated point: unlike the reach map there is no inverse_xy / translate_xy round trip.
 * rnd(v) = Rust's `v.round() as i32`: half away from zero, saturating, NaN -> 0 (the firing solutions' rounding).
 * A pixel HAS A HEIGHT iff the frame is open and has a minimap rectangle (the per-call path: a minimap was given), 0 <= rnd(px) < W
 *   and 0 <= rnd(py) < H (the firing solutions' inside test), and the z below is finite.  Everything else is flag byte 0, shade 0,
 *   height 0.0f and no paint.  (A px that is NaN rounds to 0 and is inside: NEAREST then reads texel column 0, while the bilinear
 *   weights are NaN, z is not finite and the pixel has no height.)
 * Height.  Default, bilinear: i = floor(px), fx = px - i, gx = 1.0 - fx, taps i and i + 1, each clamped into [0, W - 1]; j, fy, gy
 *   likewise from py.  With v00 = texel (i, j), v10 = (i + 1, j), v01 = (i, j + 1), v11 = (i + 1, j + 1) as f64:
 *   top = v00 * gx + v10 * fx, bot = v01 * gx + v11 * fx, v = top * gy + bot * fy.  SMHV_RELIEF_NEAREST: v = (double)texel (rnd(px),
 *   rnd(py)).  z = (v / 65535.0) * zscale, zscale = (double)scale[2] / 0.1953125 -- a true division.  With NEAREST z is "firing
 *   solutions"' height of the pixel, bit for bit, everywhere; without it wherever px and py are integers (fx = fy = 0: v = v00).
 * Neighbours.  zr = the height of pixel (X + 1, Y), zd = that of (X, Y + 1), each by the same rule also where it lies outside the window.
 * Contours (interval_m > 0; 0 = none).  L = floor((z - base_m) / interval_m).  A pair (pixel, neighbour) CROSSES iff both have a
 *   height, both L are finite and they differ.  SMHV_RELIEF_CONTOUR is set iff the right or the down pair crosses.  SMHV_RELIEF_MAJOR
 *   (major_every = M >= 1; 0 = none) is set iff for a crossing pair, lo = the lesser and hi = the greater of its two L,
 *   floor(hi / (double)M) != floor(lo / (double)M): some level index in (lo, hi] is a multiple of M, also below base_m.
 * Hillshade.  One heightmap texel is one metre on the ground, as the firing solutions' range has it.  mx = (double)W / rw,
 *   my = (double)H / rh (texels per window pixel).  p = ((zr - z) * exaggeration) / mx when the right neighbour has a height, else 0.0;
 *   q likewise from zd and my.  With light = {lx, ly, lz}, the caller's vector from the ground towards the light in heightmap axes (x
 *   right, y down, z up; not normalised by the library, no trigonometry runs on the device): t = (lz - p * lx) - q * ly,
 *   den = sqrt((1.0 + p * p) + q * q), s = t / den; !(s > 0.0) gives 0.0 and s > 1.0 gives 1.0; shade = (uint8_t)(s * 255.0 + 0.5).
 * Paint (SMHV_RELIEF_PAINT), into the batch's render slab, over whatever is there, only on pixels with a height: first the reach map's
 *   integer blend with the entry (shade, shade, shade, shade_weight), then on a CONTOUR pixel the same blend with major[4] when the
 *   MAJOR bit is set, else with contour[4].  A weight of 0 leaves the pixel as it is; the image's alpha byte is untouched.  As for
 *   the reach map the tint lies over everything already drawn; a caller draws the text passes afterwards.
 * Planes, each out_w * out_h elements per frame, rows and frames tightly packed, the call's first frame first, into caller-provided
 *   device memory (smhv_relief_planes): SMHV_RELIEF_BYTES u8 = SMHV_RELIEF_HAS_HEIGHT | _CONTOUR | _MAJOR; SMHV_RELIEF_SHADES u8;
 *   SMHV_RELIEF_HEIGHTS f32 = (float)z.  A frame without relief (closed, or no minimap rectangle) gets zeroed planes and an untouched
 *   slab.  The shade is computed when SHADES, or PAINT with shade_weight != 0, asks for it.
 * Summary.  One smhv_relief_result per frame in the batch's relief slab (allocated by the first call), cleared on the stream ahead of
 *   the kernel: valid = 1 iff the frame is open and has a minimap rectangle (else every field is 0); n_height, n_contour, n_major =
 *   window pixels with that bit; z_min, z_max = the least and the greatest z over the window pixels with a height, both 0.0 when
 *   n_height == 0. */
#define SMHV_RELIEF_PAINT 1u           /* smhv_relief_options.flags: tint the render slab (per call: implied by rgba_inout) */
#define SMHV_RELIEF_BYTES 2u           /*   ... write the flag bytes (per call: implied by bytes) */
#define SMHV_RELIEF_SHADES 4u          /*   ... write the shade bytes (per call: implied by shades) */
#define SMHV_RELIEF_HEIGHTS 8u         /*   ... write the f32 heights (per call: implied by heights) */
#define SMHV_RELIEF_NEAREST 16u        /*   ... the height is the nearest texel's, not the bilinear one */
#define SMHV_RELIEF_HAS_HEIGHT 1u      /* the flag byte */
#define SMHV_RELIEF_CONTOUR 2u
#define SMHV_RELIEF_MAJOR 4u
typedef struct {
	uint32_t size;                       /*  0: sizeof(smhv_relief_options) == 80 */
	uint32_t flags;                      /*  4: SMHV_RELIEF_PAINT | _BYTES | _SHADES | _HEIGHTS | _NEAREST (no output flag: the summary alone) */
	uint32_t major_every;                /*  8: M, every M-th level is an index contour; 0 = none */
	uint32_t reserved0;                  /* 12 */
	double interval_m;                   /* 16: metres between contour levels; 0 = none; finite, >= 0 */
	double base_m;                       /* 24: the height of level 0; finite */
	double exaggeration;                 /* 32: the slopes' factor in the hillshade; finite */
	double light[3];                     /* 40: from the ground towards the light (x right, y down, z up); finite */
	uint8_t contour[4];                  /* 64: R, G, B and the blend weight a of a contour pixel */
	uint8_t major[4];                    /* 68: ... of an index contour's pixel */
	uint32_t shade_weight;               /* 72: the blend weight of the hillshade, <= 255 */
	uint32_t reserved;                   /* 76 */
} smhv_relief_options;
typedef struct {
	uint32_t valid;                      /*  0 */
	uint32_t n_height;                   /*  4 */
	uint32_t n_contour;                  /*  8 */
	uint32_t n_major;                    /* 12 */
	double z_min;                        /* 16 */
	double z_max;                        /* 24 */
	uint32_t reserved[4];                /* 32 */
} smhv_relief_result;                    /* 48 bytes */
typedef struct {
	void *bytes;                         /*  0: SMHV_RELIEF_BYTES: n * out_w * out_h u8, device memory */
	void *shades;                        /*  8: SMHV_RELIEF_SHADES: n * out_w * out_h u8 */
	void *heights;                       /* 16: SMHV_RELIEF_HEIGHTS: n * out_w * out_h f32 */
} smhv_relief_planes;                    /* 24 bytes */
/* Host only.  Fills *opt: size, flags = PAINT, interval_m = 10, base_m = 0, major_every = 5, exaggeration = 1, light from the
 * north-west at 45 degrees {-0.5, -0.5, 0x1.6a09e667f3bcdp-1}, contour (60, 40, 20, 110), major (60, 40, 20, 200), shade_weight 96. */
SMHV_API int smhv_relief_defaults(smhv_relief_options *opt);
/* The terrain relief of frames [first, first + n), asynchronously on `stream`; the frames' results in the relief slab are cleared on
 * the stream ahead of the kernel.  ropt supplies the window and the viewport (quad, background and the HEIGHTMAP / MARKERS flags are
 * not used); hm is the terrain.  With PAINT the call runs behind whatever the batch's previous render enqueued and ropt->out_w /
 * out_h must be the most recent render's (SMHV_E_STATE for another size or before the first render).  Without PAINT only the records
 * are read: a plain batch after smhv_batch_run, or a pipeline slot's batch after smhv_pipeline_wait, for both searches (a batch that
 * has not run has closed maps only).  planes (NULL: none) names the planes' device memory.  SMHV_E_INVALID: hm == NULL (relief
 * without terrain is nothing), what smhv_batch_render rejects in ropt, a wrong size, unknown flags, a plane flag whose pointer (or
 * `planes`) is NULL, an interval_m, base_m, exaggeration or light component that is not finite, interval_m < 0, shade_weight > 255,
 * n == 0, a range beyond the batch's capacity, a heightmap on another device.  A failed call enqueues nothing.  The batch keeps a
 * reference of hm as smhv_batch_render does. */
SMHV_API int smhv_batch_relief(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *ropt,
                               const smhv_relief_options *opt, const smhv_relief_planes *planes, void *stream);
/* The batch's relief slab: read is a synchronising host copy, ptr the device address (SMHV_E_STATE before the first smhv_batch_relief) */
SMHV_API int smhv_batch_read_relief(smhv_batch *b, uint32_t first, uint32_t n, smhv_relief_result *out);
SMHV_API int smhv_batch_relief_ptr(smhv_batch *b, void **d_relief);
/* The per-call path, stateless like smhv_reach_map: minimap = {left, right, top, bottom} (NULL: none -- nothing has a height).
 * rgba_inout (host, out_w * out_h * 4 bytes, an image of any smhv_render_map* call or any other) is tinted in place; bytes, shades
 * (host, out_w * out_h bytes each) and heights (host, out_w * out_h floats) receive the planes; result receives the summary.  Each
 * of the five may be NULL, not all of them.  Of opt->flags NEAREST applies; the others are checked and otherwise not used.  Runs
 * on the context's stream. */
SMHV_API int smhv_relief_map(smhv_ctx *ctx, const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_relief_options *opt,
                             const uint32_t minimap[4], uint8_t *rgba_inout, uint8_t *bytes, uint8_t *shades, float *heights,
                             smhv_relief_result *result);

/* ---- scale labels: word boxes, the bar under each, glyph crops -----------------------------------------------------------------
 * The reference's scales branch (src/vision/mod.rs:128-193) pulls the whole ocr_preprocess plane to the host, runs a full-page OCR
 * over it (ocr::read, mod.rs:149) and filters the hits (mod.rs:161-186) into label anchors.  Reading digits stays on the host; all
 * the branch needs from the OCR besides is geometry, and this pass finds it on the device: which blobs of the plane are words, their
 * boxes, which of them have a scale bar `I-----I` beneath them and how wide that bar is.  The host reads three or four glyphs in at
 * most eight 128 x 32 crops per frame and hands the numbers to smhv_scale_labels_anchors.  Every value of the rule is an integer.
 * Per open frame, P = the frame's ocr_preprocess plane, qw x qh (brq_w x brq_h); a pixel is foreground when P != 255:
 *   gap         g = max(1, round(4.0 / 640.0 * qw)) in f64, round half away from zero (f64::round, as max_scale_y_offset of
 *               mpx_ratio.rs:12 is rounded): 1 at qw 180 and 197, 2 at 357, 4 at 657.
 *   row runs    foreground pixels of one row belong to the same run when at most g non-foreground pixels lie between neighbours; a
 *               run is [l, r], its first and last foreground pixel.  Two runs on adjacent rows touch when l1 <= r2 + 1 && l2 <= r1 + 1.
 *   words       the connected components of the runs.  Box: left = min l, top = min y, right = max r + 1, bottom = max y + 1 (right
 *               and bottom exclusive, as in the OCR hits the reference consumes).
 *   candidates  boxes with 3 <= right - left <= SMHV_LABEL_CROP_W && 3 <= bottom - top <= SMHV_LABEL_CROP_H.
 *   anchor      ((left + right) / 2, bottom), src/vision/mod.rs:181.
 *   bar         find_scale_width (mpx_ratio.rs:3-67, exactly the rule smhv_calc_meters_to_px_ratio and SMHV_STAGE_SCALES apply: pixels
 *               outside the image count as non-zero, None for y < 4, max_scale_y_offset rows are scanned) from the anchor on S0 =
 *               find_scales_preprocess with start row 0.  The scan only reads rows at or below the anchor, and a row of
 *               find_scales_preprocess is the same whatever start row at or above it the image was made with: the bar does not depend
 *               on the start row, so it is the bar a later SMHV_STAGE_SCALES run finds from this anchor (scales_start_y <= its y).
 *   proposals   candidates with a bar and bar_right > bar_left; width = bar_right - bar_left.  The u32 wrap the reference tolerates
 *               (right < left: a filled dark block under a word) is not a proposal.
 *   order, cap  ascending by (top, left, right, bottom); the first SMHV_MAX_SCALE_LABELS are written (label[] and their crops), n_found
 *               counts all of them.  (Two proposals with the same box have the same anchor, bar and crop.)
 *   header      n = min(n_found, SMHV_MAX_SCALE_LABELS), n_found, n_words = all words of the frame, candidates or not, n_runs,
 *               flags.  A frame with more than SMHV_LABEL_MAX_RUNS runs has SMHV_LABELS_RUNS_OVERFLOW set, n = n_found = n_words = 0
 *               and n_runs = the true count; nothing is written past any cap.  label[i] for i >= n is zero.  A closed frame's
 *               record is all zeros.
 *   crops       a frame has SMHV_MAX_SCALE_LABELS cells of SMHV_LABEL_CROP_W x SMHV_LABEL_CROP_H bytes, row-major; cell i < n
 *               holds the pixels of P inside label[i]'s box, placed at the cell's top-left corner, every other byte of it 255.
 *               Cells i >= n are not written.
 * The three limits are conditions, not measurements; the reference's own sample screenshots have at most 296 runs, 4 proposals and
 * boxes of 36 x 16 at 2560 x 1440. */
#define SMHV_MAX_SCALE_LABELS 8u
#define SMHV_LABEL_MAX_RUNS 4096u
#define SMHV_LABEL_CROP_W 128u
#define SMHV_LABEL_CROP_H 32u
#define SMHV_LABELS_RUNS_OVERFLOW 1u   /* smhv_scale_label_frame.flags */
typedef struct {
	uint32_t left, top, right, bottom;   /*  0: the word's box, brq coordinates; right and bottom exclusive */
	uint32_t bar_left, bar_y, bar_right; /* 16: find_scale_width's (left, y, right), the scales_debug line */
	uint32_t width;                      /* 28: bar_right - bar_left */
} smhv_scale_label;                      /* 32 bytes */
typedef struct {
	uint32_t n, n_found, n_words, n_runs; /*  0 */
	uint32_t flags;                      /* 16: SMHV_LABELS_RUNS_OVERFLOW */
	uint32_t reserved[3];                /* 20 */
	smhv_scale_label label[SMHV_MAX_SCALE_LABELS];
} smhv_scale_label_frame;                /* 288 bytes */
#define SMHV_LABEL_CROP_BYTES (SMHV_LABEL_CROP_W * SMHV_LABEL_CROP_H)                /* a cell */
#define SMHV_LABEL_FRAME_CROP_BYTES (SMHV_MAX_SCALE_LABELS * SMHV_LABEL_CROP_BYTES)  /* a frame's cells */
/* The scale labels of frames [0, n), asynchronously on `stream`, behind a run of this batch over the same frames: a plain batch after
 * smhv_batch_run, or a pipeline slot's batch after smhv_pipeline_wait.  d_frames: the frames that run was given, under
 * smhv_batch_run's contract (S0 is made from their pixels, into a plane of this family's own that the first call allocates; the
 * batch's scales plane, its ocr plane and its records are not touched).  The records go to the batch's label slab, the cells to its
 * crop slab (both allocated by the first call).
 * SMHV_E_STATE: the batch's last run had no SMHV_STAGE_OCR, or covered fewer than n frames.  SMHV_E_GEOMETRY: a quadrant wider or
 * taller than 2048 pixels.  SMHV_E_INVALID: null or misaligned d_frames, n == 0 or beyond the batch's capacity.  A failed call
 * enqueues nothing. */
SMHV_API int smhv_batch_scale_labels(smhv_batch *b, const void *d_frames, uint32_t n, void *stream);
/* The batch's label and crop slabs: read is a synchronising host copy of frames [first, first + n) -- out: n records, crops (NULL:
 * none): n * SMHV_LABEL_FRAME_CROP_BYTES bytes; ptr the device addresses, either may be NULL (SMHV_E_STATE before the first
 * smhv_batch_scale_labels). */
SMHV_API int smhv_batch_read_scale_labels(smhv_batch *b, uint32_t first, uint32_t n, smhv_scale_label_frame *out, uint8_t *crops);
SMHV_API int smhv_batch_scale_labels_ptr(smhv_batch *b, void **d_labels, void **d_crops);
/* The per-call form, on the frame of the context's last smhv_ocr_preprocess (SMHV_E_STATE before it, or with the map closed): out
 * receives the record, crops (NULL: none) SMHV_LABEL_FRAME_CROP_BYTES bytes, of which the cells i >= out->n are left as they are. */
SMHV_API int smhv_scale_labels(smhv_ctx *ctx, smhv_scale_label_frame *out, uint8_t *crops);
/* Host only: the label filter of src/vision/mod.rs:161-186 and the ladder of mpx_ratio.rs:91-125 on what the host has read.
 * labels: n records in OCR order (the order of label[]), meters[i]: the number read in label i's crop, 0: "not a label" (what the
 * reference skips: no trailing m, not a number, zero).  *out (optional) receives the anchors of a SMHV_STAGE_SCALES run: the first
 * SMHV_MAX_SCALES distinct non-zero values in order, {meters, (left + right) / 2, bottom} each, and scales_start_y = the minimum
 * bottom over the non-zero entries met up to and including the one that filled the list (the reference's loop breaks there);
 * n = 0, scales_start_y = 0 when there is none.  *mpx, *has (optional): the mean of meters / width over those anchors, summed in
 * order -- every anchor taken here has a bar, so this is the record's mpx after that run, bit for bit; *has = 0: no anchor. */
SMHV_API int smhv_scale_labels_anchors(const smhv_scale_label *labels, uint32_t n, const uint32_t *meters, smhv_anchors *out, double *mpx, int *has);

/* ---- scale labels: text -- the glyphs of a label read on the device against the caller's glyph atlas ------------------------------
 * A label is a handful of glyphs of one fixed font at the caller's resolution.  The library ships no glyph shapes: a caller who has
 * read one frame's labels once (by eye, with an OCR engine, through label_reader=) turns them into templates with
 * smhv_glyph_templates_from_label, and every later frame is read on the device.  The rule (csrc/smh_glyph_rule.h is its one text,
 * for the kernel, the host helpers and a stand-alone check), integers only:
 *   input      label i < n of a smhv_scale_label_frame and its cell; w = right - left, h = bottom - top.  Foreground is P != 255.  Only
 *              columns [0, w) and rows [0, h) of the cell are looked at (w <= 128, h <= 32 by the candidates' limits).
 *   glyphs     the maximal runs of columns that hold a foreground pixel, left to right.  A glyph's bitmap is its tight box: the run's
 *              columns, from the first to the last non-empty row inside the run.  A label with more than SMHV_LABEL_MAX_GLYPHS glyphs
 *              has SMHV_LABEL_TEXT_TOO_MANY set, n_glyphs = the true count, and nothing else: empty text, meters 0, every per-glyph
 *              field 0.  A glyph wider than 32 columns is unmatched: character '?', best = second = 0xFFFF, tmpl = 0xFF.
 *   template   smhv_glyph_template: bit x of rows[y] is foreground.  code is printable ASCII 0x21 .. 0x7E and not '?';
 *              1 <= w, h <= 32; the box is tight (row 0, row h - 1, column 0 and column w - 1 are non-empty) and no bit lies outside
 *              it (rows[y] for y >= h is 0).  An atlas holds 1 .. SMHV_ATLAS_MAX_TEMPLATES templates; several may share a code.
 *   distance   of glyph G to template T: the minimum over (dx, dy) in {-1, 0, 1}^2 of the number of positions of the plane at which
 *              G moved by (dx, dy) differs from T.  Both are anchored at their box's top-left corner; everything outside a box is
 *              background.  (The shifts are taken dy-major, dx-minor; only the minimum is kept.)
 *   choice     the winner is the template of least distance, ties to the lowest index; best = its distance.  second = the least
 *              distance over the templates whose code differs from the winner's (0xFFFF: none).  The glyph is accepted when
 *              best * accept_den <= accept_num * fg(winner) in u32 arithmetic, fg = the template's foreground count; the defaults are
 *              1 and 3.  An accepted glyph prints the winner's code, any other '?' -- best, second and tmpl are kept either way.
 *   meters     the filter of src/vision/mod.rs:161-173 on the text: p = rfind('m'); text[0, p) must parse as u32::from_str does (an
 *              optional single '+', then one or more digits, no overflow); anything else -- no 'm', an empty prefix, another
 *              character (a '?' among them), a value above 4294967295 -- is 0, and so is the value 0.  What follows the last 'm' is
 *              ignored, as the reference ignores it.
 *   frame      smhv_scale_labels_anchors' rule on the meters just read, labels in order: anchors, has, mpx (the mean of
 *              meters / width summed in order in f64; 0.0 when has == 0).  A closed frame or a SMHV_LABELS_RUNS_OVERFLOW frame has
 *              n = 0 labels: its record is all zeros.
 * label[i] for i >= n, and every per-glyph field k >= min(n_glyphs, SMHV_LABEL_MAX_GLYPHS), is zero. */
#define SMHV_LABEL_MAX_GLYPHS 16u
#define SMHV_ATLAS_MAX_TEMPLATES 32u
#define SMHV_LABEL_TEXT_TOO_MANY 1u      /* smhv_label_text_entry.flags */
typedef struct {
	uint8_t code, w, h, reserved;        /*  0 */
	uint32_t rows[32];                   /*  4: bit x of rows[y] */
} smhv_glyph_template;                   /* 132 bytes */
typedef struct {
	uint32_t accept_num, accept_den;     /* accepted: best * accept_den <= accept_num * fg(winner); defaults 1, 3 */
} smhv_glyph_atlas_options;
typedef struct {
	char text[SMHV_LABEL_MAX_GLYPHS];    /*  0: a character per glyph, zero-padded (16 glyphs: no terminator) */
	uint32_t n_glyphs;                   /* 16: the true count */
	uint32_t flags;                      /* 20: SMHV_LABEL_TEXT_TOO_MANY */
	uint32_t meters;                     /* 24: 0: not a label */
	uint32_t reserved;                   /* 28 */
	uint16_t best[SMHV_LABEL_MAX_GLYPHS];   /* 32 */
	uint16_t second[SMHV_LABEL_MAX_GLYPHS]; /* 64 */
	uint8_t tmpl[SMHV_LABEL_MAX_GLYPHS];    /* 96: the winner's index in the atlas */
} smhv_label_text_entry;                    /* 112 bytes */
typedef struct {
	uint32_t n;                          /*  0: the labels of the frame (smhv_scale_label_frame.n) */
	uint32_t has;                        /*  4: 1: anchors.n > 0, mpx is a number */
	double mpx;                          /*  8 */
	smhv_anchors anchors;                /* 16: 44 bytes */
	uint32_t reserved;                   /* 60 */
	smhv_label_text_entry label[SMHV_MAX_SCALE_LABELS]; /* 64 */
} smhv_label_text_frame;                 /* 960 bytes */
#ifdef __cplusplus
static_assert(sizeof(smhv_glyph_template) == 132 && sizeof(smhv_anchors) == 44, "glyph template / anchors layout");
static_assert(sizeof(smhv_label_text_entry) == 112 && offsetof(smhv_label_text_entry, n_glyphs) == 16 && offsetof(smhv_label_text_entry, meters) == 24 &&
              offsetof(smhv_label_text_entry, best) == 32 && offsetof(smhv_label_text_entry, second) == 64 && offsetof(smhv_label_text_entry, tmpl) == 96, "smhv_label_text_entry layout");
static_assert(sizeof(smhv_label_text_frame) == 960 && offsetof(smhv_label_text_frame, mpx) == 8 && offsetof(smhv_label_text_frame, anchors) == 16 &&
              offsetof(smhv_label_text_frame, label) == 64, "smhv_label_text_frame layout");
#endif
typedef struct smhv_glyph_atlas smhv_glyph_atlas;
/* Host only: are these n templates an atlas (the conditions under "template", 1 <= n <= SMHV_ATLAS_MAX_TEMPLATES)?  SMHV_E_INVALID
 * names the first template that is not. */
SMHV_API int smhv_glyph_templates_check(const smhv_glyph_template *templates, uint32_t n);
/* Host only, the learning helper: cuts one label by the rule (crop: its cell of SMHV_LABEL_CROP_BYTES bytes) and pairs glyph k with
 * text[k]; out receives *n templates (room for SMHV_LABEL_MAX_GLYPHS).  SMHV_E_INVALID: the glyph count differs from strlen(text) or
 * exceeds SMHV_LABEL_MAX_GLYPHS, a glyph is wider than 32 columns, a character is not allowed as a code, a box larger than a cell. */
SMHV_API int smhv_glyph_templates_from_label(const uint8_t *crop, const smhv_scale_label *label, const char *text, smhv_glyph_template *out, uint32_t *n);
/* A device-resident atlas, like smhv_heightmap: usable by every batch, pipeline slot and per-call path of its context's device until
 * destroyed (destroy waits for the device).  options NULL: the defaults.  SMHV_E_INVALID: what smhv_glyph_templates_check rejects,
 * accept_den == 0. */
SMHV_API int smhv_glyph_atlas_create(smhv_ctx *ctx, const smhv_glyph_template *templates, uint32_t n, const smhv_glyph_atlas_options *options, smhv_glyph_atlas **out);
SMHV_API void smhv_glyph_atlas_destroy(smhv_glyph_atlas *atlas);
/* The texts of frames [0, n), asynchronously on `stream`, behind smhv_batch_scale_labels of this batch over at least n frames
 * (SMHV_E_STATE otherwise) -- a plain batch, or a pipeline slot's batch after smhv_pipeline_wait.  The records go to the batch's text
 * slab, the frames' anchors tightly packed to its label-anchor slab (both allocated by the first call).  SMHV_E_INVALID: null
 * arguments, n == 0 or beyond the batch's capacity, an atlas of another device.  A failed call enqueues nothing. */
SMHV_API int smhv_batch_label_text(smhv_batch *b, const smhv_glyph_atlas *atlas, uint32_t n, void *stream);
/* read: a synchronising host copy of the records of frames [first, first + n); ptr: the device addresses of the text slab and of the
 * smhv_anchors array, either may be NULL (SMHV_E_STATE before the first smhv_batch_label_text). */
SMHV_API int smhv_batch_read_label_text(smhv_batch *b, uint32_t first, uint32_t n, smhv_label_text_frame *out);
SMHV_API int smhv_batch_label_text_ptr(smhv_batch *b, void **d_text, void **d_anchors);
/* The per-call form, after smhv_scale_labels on the same frame (SMHV_E_STATE otherwise). */
SMHV_API int smhv_label_text(smhv_ctx *ctx, const smhv_glyph_atlas *atlas, smhv_label_text_frame *out);
/* smhv_batch_run with the anchors the batch's last smhv_batch_label_text wrote (SMHV_E_STATE: none, or over fewer than n frames):
 * where smhv_batch_run copies the caller's anchors from pinned staging, this copies the label-anchor slab device to device on the
 * same stream; nothing else of the run differs, so the records equal those of smhv_batch_run given the same anchors by the host.
 * The frames' meters never visit the host.  (Pipelines take host anchors only.) */
SMHV_API int smhv_batch_run_label_anchors(smhv_batch *b, const void *d_frames, uint32_t n, uint32_t stages, int grayscale, uint32_t max_gap, void *stream);

/* ---- map grid: grid lines, cell labels and keypad references of every window pixel and of the line ends ----------------------------
 * A mortar team talks in grid references: "B4, keypad 7, sub-keypad 3".  In Squad the minimap rectangle is the whole map and the
 * grid's A1 sits at its top-left corner; with metres per pixel the cell of every window pixel and of every point follows.  The
 * reference draws no grid; the rectangle and the translated points are "firing solutions"' alone.  Every operation is one IEEE f64
 * operation, left to right, unfused, but for the rectangle, which stays f32 (csrc/smh_grid.h is the rule's one text, for the
 * kernels, the host helper and a stand-alone check).
 * Rectangle.  R = {l, t, r, b} = the heightmap's rectangle of "firing solutions" in f32, from the frame's minimap rectangle through the
 *   render options' viewport (viewport_scale, 0 = 1; viewport_top_left).  An axis is (r0, r1) = (l, r) or (t, b), rlen = (double)(r1 - r0),
 *   the difference in f32, s = the axis' viewport scale.
 * Source.  SMHV_GRID_HEIGHTMAP: a heightmap is given and the frame is open and has a minimap rectangle (per call: a minimap was
 *   given); SMHV_RENDER_BOUNDS_OFFSET acts on R as in the relief.  Metres of an f32 coordinate c on an axis of n texels:
 *   m = (((double)c - (double)r0) / rlen) * (double)n -- one texel is one metre -- and pixels per metre ppm = rlen / (double)n.
 *   SMHV_GRID_SCALES: no heightmap; the frame is open, has a minimap rectangle and metres per pixel (the record's has_mpx / mpx; per
 *   call the mpx argument); no bounds offset applies.  m = (((double)c - (double)r0) / (double)s) * mpx, ppm = (double)s / mpx.
 *   SMHV_GRID_NONE: anything else; nothing has a cell, the planes are zero and the summary is zero.
 * Axis.  g = m - origin_m[axis].  The coordinate is IN iff r0 <= c && c < r1 in f32 and g is finite.  L = levels (0 .. 3),
 *   P3 = {1, 3, 9, 27}, size_k = cell_m / (double)P3[k], a true division.  qf = floor(g / size_L), the one division of an axis
 *   entry; the coordinate has no index when g is not finite or qf lies outside [-2^31, 2^31).  idx_L = (int64)qf, and every coarser
 *   index comes by integer floor division, idx_(k-1) = floor_div(idx_k, 3) (towards minus infinity): a cell and its keypads agree by
 *   construction, no second division exists that could disagree with the first at a boundary.
 * Cell.  A pixel (c = X + 0.5f, Y + 0.5f in f32) or a point HAS A CELL iff both axes are IN and have an index, col = idx_0(x) lies
 *   in [0, 702) and row1 = idx_0(y) + 1 in [1, 999].  Keypad digit of level k >= 1: cx = idx_k(x) mod 3, cy = idx_k(y) mod 3
 *   (non-negative), digit = (2 - cy) * 3 + cx + 1: 7 8 9 on the top row as on the in-game map.
 * Text.  The column in bijective base 26 (A .. Z, AA .. ZZ), the row in decimal, then "-<digit>" per level: "B4-7-3"; at most 11
 *   characters, NUL-padded to 16.
 * Drawn levels.  Ld = the greatest k <= L with size_k * ppm_x >= min_px and size_k * ppm_y >= min_px; -1 when no k does.
 * Lines.  The pair (pixel, right neighbour), both with a cell, CROSSES at the least k <= Ld at which their idx_k(x) differ; the pair
 *   (pixel, down neighbour) likewise with y.  A neighbour is evaluated by the same rule also where it lies outside the window.  The
 *   pixel's line level is the lesser of its two pairs' levels, or none.
 * Cell label.  "<letters><row>" inside every cell, in the 5 x 7 font of smhv_text_font, when Ld >= 0, label[3] != 0, rlen > 0 on both
 *   axes and size_0 * ppm >= label_min_px on both.  Xfirst = the least integer column, inside the window or not, whose axis entry has
 *   the pixel's own idx_0(x); Yfirst likewise.  ox = X - Xfirst - 3, oy = Y - Yfirst - 3; glyph gi = ox div 6, its column ox mod 6
 *   (< 5), its row oy (0 .. 6), gi < the label's length; a pixel with a cell is LIT iff the font has that bit.  ox comes from the
 *   pixel's own cell, so a label is clipped by its cell.  (A label is at most 5 glyphs: columns more than 32 to the left of X
 *   decide nothing and are not looked at.)
 * Paint (SMHV_GRID_PAINT), into the batch's render slab over whatever is there: the reach map's integer blend with line[k] on a pixel
 *   of line level k (0 = major .. 3 = sub-sub-keypad), then with label on a LIT pixel.  A weight of 0 leaves the pixel as it is; the
 *   alpha byte is untouched.
 * Planes, out_w * out_h elements per frame, rows and frames tightly packed, the call's first frame first, into caller-provided device
 *   memory (smhv_grid_planes): SMHV_GRID_BYTES u8 = SMHV_GRID_HAS_CELL | (level + 1) << 1 | SMHV_GRID_LABEL; SMHV_GRID_CELLS u32 =
 *   col | row1 << 10 | digit_1 << 20 | digit_2 << 24 | digit_3 << 28, digits beyond `levels` 0, the whole word 0 without a cell.
 * Summary.  One smhv_grid_result per frame in the batch's grid slab, cleared on the stream ahead of the kernel: valid = 1 iff source
 *   != NONE (else every field is 0), source, drawn_levels = Ld + 1, n_cell, n_line[k], n_label = window pixels with a cell, of line
 *   level k, LIT; col_first / col_last = the least and the greatest col, row_first / row_last the least and the greatest row1 over
 *   the window pixels with a cell, all 0 when n_cell == 0.
 * References (smhv_batch_grid_refs / smhv_grid_refs).  Each end of a line is the point P = (x * sw + tx, y * sh + ty) in f32, as the
 *   firing solutions translate it, through the same axis rule: x_m, y_m = the g of both axes (0.0 where g is not finite), valid,
 *   col, row1, digit[k - 1] and the text; a point without a cell has valid = 0 and zeros there.  With source NONE every field is 0. */
#define SMHV_GRID_PAINT 1u             /* smhv_grid_options.flags: draw into the render slab (per call: implied by rgba_inout) */
#define SMHV_GRID_BYTES 2u             /*   ... write the flag bytes (per call: implied by bytes) */
#define SMHV_GRID_CELLS 4u             /*   ... write the cell words (per call: implied by cells) */
#define SMHV_GRID_HAS_CELL 1u          /* the flag byte; bits 1 .. 3 = line level + 1 */
#define SMHV_GRID_LABEL 0x10u
#define SMHV_GRID_NONE 0u              /* smhv_grid_result.source */
#define SMHV_GRID_SCALES 1u
#define SMHV_GRID_HEIGHTMAP 2u
#define SMHV_GRID_MAX_COLS 702u        /* A .. ZZ */
#define SMHV_GRID_MAX_ROWS 999u
typedef struct {
	uint32_t size;                       /*  0: sizeof(smhv_grid_options) == 80 */
	uint32_t flags;                      /*  4: SMHV_GRID_PAINT | _BYTES | _CELLS (no output flag: the summary alone) */
	uint32_t levels;                     /*  8: L, keypad levels below the cell, 0 .. 3 */
	uint32_t reserved0;                  /* 12 */
	double cell_m;                       /* 16: the side of a cell in metres; finite, > 0 */
	double origin_m[2];                  /* 24: metres from the rectangle's top-left corner to the corner of A1; finite */
	double min_px;                       /* 40: a level is drawn when its cells are at least this many pixels wide and high; finite, >= 0 */
	double label_min_px;                 /* 48: ... the labels when the cells are; finite */
	uint8_t line[4][4];                  /* 56: R, G, B and the blend weight a of a line pixel of level 0 .. 3 */
	uint8_t label[4];                    /* 72: ... of a LIT pixel; a == 0: no labels */
	uint32_t reserved;                   /* 76 */
} smhv_grid_options;
typedef struct {
	uint32_t valid;                      /*  0 */
	uint32_t source;                     /*  4 */
	uint32_t drawn_levels;               /*  8: Ld + 1 */
	uint32_t n_cell;                     /* 12 */
	uint32_t n_line[4];                  /* 16 */
	uint32_t n_label;                    /* 32 */
	uint32_t col_first, col_last;        /* 36 */
	uint32_t row_first, row_last;        /* 44: as row1 */
	uint32_t reserved[3];                /* 52 */
} smhv_grid_result;                      /* 64 bytes */
typedef struct {
	void *bytes;                         /*  0: SMHV_GRID_BYTES: n * out_w * out_h u8, device memory */
	void *cells;                         /*  8: SMHV_GRID_CELLS: n * out_w * out_h u32 */
} smhv_grid_planes;                      /* 16 bytes */
typedef struct {
	double x_m, y_m;                     /*  0: g of both axes */
	uint32_t col, row1;                  /* 16 */
	uint8_t digit[3];                    /* 24: the keypad digits of levels 1 .. 3, 0 beyond `levels` */
	uint8_t valid;                       /* 27: the point has a cell */
	uint32_t reserved;                   /* 28 */
	char text[16];                       /* 32 */
} smhv_grid_ref;                         /* 48 bytes */
typedef struct {
	uint32_t n_lines;                    /*  0 */
	uint32_t source;                     /*  4 */
	uint32_t reserved[2];                /*  8 */
	smhv_grid_ref ref[SMHV_MAX_LINES][2]; /* 16: the line's first and second end */
} smhv_grid_refs_result;                 /* 3088 bytes */
#ifdef __cplusplus
static_assert(sizeof(smhv_grid_options) == 80 && sizeof(smhv_grid_result) == 64 && sizeof(smhv_grid_planes) == 16, "map grid layout");
static_assert(sizeof(smhv_grid_ref) == 48 && sizeof(smhv_grid_refs_result) == 3088, "map grid references layout");
#endif
/* Host only.  Fills *opt: size, flags = PAINT, cell_m = 300, levels = 2, origin_m = {0, 0}, min_px = 12, label_min_px = 48, line =
 * (0, 0, 0, 170), (0, 0, 0, 110), (0, 0, 0, 70), (0, 0, 0, 45), label = (0, 0, 0, 200). */
SMHV_API int smhv_grid_defaults(smhv_grid_options *opt);
/* Host only: the text of a reference; digits[k - 1] = the digit of level k, levels of them are printed (digits may be NULL when
 * levels == 0).  SMHV_E_INVALID: col >= 702, row1 outside 1 .. 999, levels > 3, a digit outside 1 .. 9, out == NULL. */
SMHV_API int smhv_grid_ref_text(uint32_t col, uint32_t row1, const uint8_t *digits, uint32_t levels, char out[16]);
/* The grid of frames [first, first + n), asynchronously on `stream`; the frames' results in the grid slab are cleared on the stream
 * ahead of the kernel.  ropt supplies the window and the viewport; hm: the heightmap branch, NULL: the scales branch.  With PAINT
 * the call runs behind whatever the batch's previous render enqueued and ropt->out_w / out_h must be the most recent render's
 * (SMHV_E_STATE otherwise); without it only the records are read, as smhv_batch_relief reads them.  SMHV_E_INVALID: a wrong size,
 * unknown flags, a plane flag whose pointer (or `planes`) is NULL, cell_m not finite or <= 0, levels > 3, origin_m, min_px or
 * label_min_px not finite, min_px < 0, what smhv_batch_render rejects in ropt, n == 0, a range beyond the batch's capacity, a
 * heightmap on another device.  A failed call enqueues nothing.  The batch keeps a reference of hm as smhv_batch_render does. */
SMHV_API int smhv_batch_grid(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *ropt,
                             const smhv_grid_options *opt, const smhv_grid_planes *planes, void *stream);
/* The batch's grid slab: read is a synchronising host copy, ptr the device address (SMHV_E_STATE before the first smhv_batch_grid) */
SMHV_API int smhv_batch_read_grid(smhv_batch *b, uint32_t first, uint32_t n, smhv_grid_result *out);
SMHV_API int smhv_batch_grid_ptr(smhv_batch *b, void **d_grid);
/* The per-call path, stateless like smhv_relief_map: mpx (NULL: none) and minimap = {left, right, top, bottom} (NULL: none) are the
 * frame's.  rgba_inout (host, out_w * out_h * 4 bytes) is drawn into in place; bytes (host, out_w * out_h) and cells (host, out_w *
 * out_h u32) receive the planes; result the summary.  Each of the four may be NULL, not all of them.  opt->flags is checked and
 * otherwise not used.  Runs on the context's stream. */
SMHV_API int smhv_grid_map(smhv_ctx *ctx, const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_grid_options *opt, const double *mpx,
                           const uint32_t minimap[4], uint8_t *rgba_inout, uint8_t *bytes, uint32_t *cells, smhv_grid_result *result);
/* The references of the ends of the detected lines of frames [first, first + n), asynchronously on `stream`, into the batch's
 * references slab (allocated by the first call): n_lines = the record's, ref[i] = line i's two ends, every entry past n_lines zero;
 * a frame with source NONE is all zeros but n_lines.  The checks are smhv_batch_grid's (opt->flags is checked and not used). */
SMHV_API int smhv_batch_grid_refs(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *ropt,
                                  const smhv_grid_options *opt, void *stream);
SMHV_API int smhv_batch_read_grid_refs(smhv_batch *b, uint32_t first, uint32_t n, smhv_grid_refs_result *out);
SMHV_API int smhv_batch_grid_refs_ptr(smhv_batch *b, void **d_grid_refs);
/* The per-call form, shaped like smhv_firing_solutions: lines in map-ROI coordinates, out receives 2 * n references (line i's ends at
 * out[2 * i], out[2 * i + 1]); n == 0 does nothing. */
SMHV_API int smhv_grid_refs(smhv_ctx *ctx, const smhv_line *lines, uint32_t n, const double *mpx, const uint32_t minimap[4], const smhv_heightmap *hm,
                            const smhv_render_options *ropt, const smhv_grid_options *opt, smhv_grid_ref *out);

/* ---- ballistics: firing solutions and a reach map for a caller-supplied weapon ------------------------------------------------------
 * "firing solutions", "reach map" and "terrain clearance" assume one weapon (the reference's mortar: one muzzle velocity, the high
 * arc, NATO mils).  This family takes the weapon from the caller: a muzzle velocity, a gravity, the arc it is laid on, the unit its
 * sight reads, the limits of its mount, a minimum range and a dispersion cone; and it gives, beside the elevation, what a firing
 * table carries: time of flight, the arc's highest point, the angle of fall.  The library ships NO weapon table (as it ships no glyph
 * shapes); smhv_weapon_defaults is the reference's mortar and nothing else.  The reference has no such code; the solution's
 * discriminant is squadex::milliradians::calc's.  Every operation below is ONE IEEE f64 operation, left to right, unfused; the only
 * function that is not correctly rounded everywhere is the atan of the elevation itself.  Everything else a device gives is bit-equal
 * to what smhv_ballistic_solve gives on the host.
 * The weapon in the rule's terms (smhv_weapon_thresholds, computed on the host once per call, never on the device):
 *   V = velocity, g = gravity, V2 = pow(V, 2.0), V4 = pow(V, 4.0) by the C library's pow (how "firing solutions" documents its
 *   constants; for smhv_weapon_defaults they ARE those constants, 0x1.79602562a02dfp+13 and 0x1.1626291c459a8p+27, bit for bit).
 *   U = the unit's size of a degree: 360.0 / 6400.0 (SMHV_ANGLE_MILS6400), 360.0 / 6000.0 (_MILS6000); _DEGREES has none.
 *   rad(e) of an angle e in the weapon's unit = (e * U) * (pi / 180.0), in degrees e * (pi / 180.0), pi / 180.0 the f64 constant
 *   0x1.1df46a2529d39p-6.  tanlim(e) = +inf when rad(e) >= 0x1.921fb54442d18p+0 (a quarter turn or more: no limit), -inf when
 *   rad(e) <= -0x1.921fb54442d18p+0, else the C library's tan(rad(e)).
 *   t_min = tanlim(elev_min), t_max = tanlim(elev_max); B_j = tanlim(elev_min + ((elev_max - elev_min) * (double)(j + 1)) / 8.0),
 *   j = 0 .. 6: eight bands of equal width in the weapon's unit; t_disp = tan(dispersion).
 * A solution from (m, alt) = (range, altitude of the target over the muzzle), both arcs (smhv_ballistic_solve, k_ballistic_lines):
 *   disc = V4 - g * (g * (m * m) + 2.0 * alt * V2);  s = sqrt(disc);  gm = g * m;
 *   T_hi = (V2 + s) / gm (arc[SMHV_ARC_HIGH]),  T_lo = (V2 - s) / gm (arc[SMHV_ARC_LOW]); per arc, with its T and tt = T * T:
 *   elevation = atan(T) * (180.0 / pi), then / U for the mil units (for MILS6400 this is calc's expression, operation for operation);
 *   tof   = (m * sqrt(1.0 + tt)) / V                     seconds;
 *   apex  = (V2 * tt) / ((1.0 + tt) * (2.0 * g))         metres above the muzzle; 0.0 when T <= 0.0 (the arc only falls);
 *   fall  = (gm * (1.0 + tt)) / V2 - T                   the tangent of the angle of fall (positive: descending at the target);
 *   along = fabs(((m * (1.0 - (gm * T) / V2)) * (1.0 + tt)) / fall) * t_disp   the along-range half width at the target: the range's
 *           derivative by the elevation, dm/dT = m (1 - g m T / V2) / fall and dT = (1 + tt) d(angle), times the cone's half angle
 *           taken as its tangent;  cross = m * t_disp, the cross-range half width (one per solution, not per arc).
 *   status: SMHV_BAL_OUT_OF_RANGE iff !(disc >= 0.0) (disc < 0 or NaN: exactly the reach map's rule); SMHV_BAL_BELOW_MIN_RANGE iff
 *   m < range_min; and only without OUT_OF_RANGE: SMHV_BAL_ELEV_LOW iff !(T >= t_min), SMHV_BAL_ELEV_HIGH iff !(t_max >= T).  The
 *   mount's limits are decided on T, never on the elevation.  band = the number of j with T >= B_j (0 .. 7).
 *   Edges, none of them a special case -- IEEE arithmetic decides: OUT_OF_RANGE makes s NaN and with it T and every number of both
 *   arcs (band 0).  disc == 0.0: both arcs are equal in every field.  NaN in m or alt, m or alt = +inf: OUT_OF_RANGE; alt = -inf:
 *   T_hi = +inf, T_lo = -inf.  m == 0.0: gm = 0.0, T_hi = +inf (elevation a quarter turn; tof, apex, fall and along NaN), T_lo
 *   = (V2 - s) / 0.0 is an infinity or, where s == V2, NaN -- and a NaN T that is not OUT_OF_RANGE has ELEV_LOW and ELEV_HIGH both.
 *   A target far enough below makes T_lo negative: a negative elevation, apex 0.0.
 * smhv_weapon_check refuses (SMHV_E_INVALID): a wrong size, an unknown arc or unit, velocity or gravity not finite or <= 0,
 *   elev_min or elev_max not finite, elev_min > elev_max, range_min or dispersion negative or not finite.
 * Lines (smhv_batch_ballistics / smhv_ballistic_lines): source, meters and alt_delta of a line are smhv_firing_solutions' (the same
 *   device function is called); dir[0] fires from p0 at p1 with alt = alt_delta, dir[1] the reverse with -alt_delta; source NONE leaves
 *   the record zero but for `source`.  A record is 256 bytes.
 * Map (smhv_batch_ballistic_map / smhv_ballistic_map): target, origin, source, m and alt of window pixel (X, Y) are "reach map"'s, word
 *   for word.  Per pixel, T = the root of the WEAPON'S arc (smhv_weapon.arc):
 *   class byte   0 nothing (no origin, source NONE, a coordinate not finite, m NaN); 1 SMHV_BMAP_OUT_OF_RANGE; 2 _BELOW_MIN_RANGE;
 *                3 _ELEV_LOW; 4 _ELEV_HIGH (the first of these that the status has, in this order); else 5 + band (SMHV_BMAP_BAND0).
 *     | 0x80     an isochrone (SMHV_BMAP_ISO), only when iso_s > 0 and the class is not 0: b = floor(tof / iso_s); set iff b is not
 *                NaN and differs from b of pixel (X + 1, Y) or of pixel (X, Y + 1), each evaluated by the same rule even where it lies
 *                outside the window.  A neighbour whose source differs from this pixel's, whose class would be 0 or whose b is NaN
 *                does not count ("reach map"'s ring rule on the time of flight).
 *   tof plane    (SMHV_BMAP_TOF) f32 per pixel: (float)tof, the f64 value rounded once, where the class is 2 or more; NaN where it
 *                is 0 or 1 (no solution).
 *   paint        (SMHV_BMAP_PAINT) "reach map"'s integer blend with pal[class - 1], then on an isochrone pixel with iso.
 *   summary      one smhv_ballistic_map_result per frame: valid, origin as "reach map"; count[c - 1] = window pixels of class c
 *                (isochrone bit ignored), c = 1 .. 12; iso = pixels with the bit; n_tof = window pixels of class >= 5 whose tof is
 *                not NaN, tof_min / tof_max = the least and greatest tof among them (0.0 when n_tof == 0); source_mask as "reach map". */
#define SMHV_ARC_HIGH 0u               /* smhv_weapon.arc; also the index into smhv_ballistic_solution.arc */
#define SMHV_ARC_LOW 1u
#define SMHV_ANGLE_MILS6400 0u         /* smhv_weapon.unit */
#define SMHV_ANGLE_MILS6000 1u
#define SMHV_ANGLE_DEGREES 2u
#define SMHV_BAL_OUT_OF_RANGE 1u       /* smhv_ballistic_arc.status */
#define SMHV_BAL_BELOW_MIN_RANGE 2u
#define SMHV_BAL_ELEV_LOW 4u
#define SMHV_BAL_ELEV_HIGH 8u
#define SMHV_BMAP_PAINT 1u             /* smhv_ballistic_options.flags: tint the render slab (per call: implied by rgba_inout) */
#define SMHV_BMAP_CLASSES 2u           /*   ... write the class bytes (per call: implied by classes) */
#define SMHV_BMAP_TOF 4u               /*   ... write the time-of-flight plane (per call: implied by tof) */
#define SMHV_BMAP_OUT_OF_RANGE 1u      /* the class byte */
#define SMHV_BMAP_BELOW_MIN_RANGE 2u
#define SMHV_BMAP_ELEV_LOW 3u
#define SMHV_BMAP_ELEV_HIGH 4u
#define SMHV_BMAP_BAND0 5u
#define SMHV_BMAP_ISO 0x80u
typedef struct {
	uint32_t size;                       /*  0: sizeof(smhv_weapon) == 80 */
	uint32_t arc;                        /*  4: SMHV_ARC_*: the arc the weapon is laid on */
	uint32_t unit;                       /*  8: SMHV_ANGLE_* */
	uint32_t reserved0;                  /* 12: 0 */
	double velocity;                     /* 16: m/s */
	double gravity;                      /* 24: m/s^2, the weapon's gravity scale multiplied in */
	double elev_min, elev_max;           /* 32, 40: the mount's limits, in the weapon's unit */
	double range_min;                    /* 48: metres */
	double dispersion;                   /* 56: the cone's half angle, radians; 0 = none */
	uint32_t reserved[4];                /* 64: 0 */
} smhv_weapon;
typedef struct {
	double v, g, v2, v4;                 /*  0 */
	double t_min, t_max;                 /* 32 */
	double band[7];                      /* 48: B_j */
	double t_disp;                       /* 104 */
	double range_min;                    /* 112 */
	double unit_deg;                     /* 120: U; 1.0 for SMHV_ANGLE_DEGREES */
	uint32_t arc, unit;                  /* 128 */
} smhv_weapon_rule;                      /* 136 bytes */
typedef struct {
	double elevation;                    /*  0: in the weapon's unit */
	double tof;                          /*  8 */
	double apex;                         /* 16 */
	double fall;                         /* 24 */
	double along;                        /* 32 */
	uint32_t status;                     /* 40: SMHV_BAL_* */
	uint32_t band;                       /* 44 */
} smhv_ballistic_arc;                    /* 48 bytes */
typedef struct {
	double meters;                       /*  0 */
	double alt_delta;                    /*  8: the target over the muzzle, as this direction sees it */
	double cross;                        /* 16 */
	uint32_t source;                     /* 24: SMHV_FIRING_NONE / _SCALES / _HEIGHTMAP (smhv_ballistic_solve: 0) */
	uint32_t reserved;                   /* 28 */
	smhv_ballistic_arc arc[2];           /* 32: [SMHV_ARC_HIGH], [SMHV_ARC_LOW] */
} smhv_ballistic_solution;               /* 128 bytes */
typedef struct { smhv_ballistic_solution dir[2]; } smhv_ballistic;   /* 256 bytes: [0] from p0 at p1, [1] from p1 at p0 */
typedef struct {
	uint32_t n_lines, reserved[3];       /* == the record's n_lines; lines beyond it are zero */
	smhv_ballistic line[SMHV_MAX_LINES]; /* 16 */
} smhv_ballistic_result;
typedef struct {
	uint32_t size;                       /*  0: sizeof(smhv_ballistic_options) == 96 */
	uint32_t flags;                      /*  4: SMHV_BMAP_PAINT | _CLASSES | _TOF (0: the summary alone) */
	uint32_t origin_mode;                /*  8: SMHV_REACH_ORIGIN_* */
	uint32_t line;                       /* 12: _LINE_P0 / _LINE_P1: which line of the record, < SMHV_MAX_LINES */
	float origin[2];                     /* 16: _POINT: the origin, map-ROI coordinates */
	double iso_s;                        /* 24: seconds between isochrones; 0 = none; finite, >= 0 */
	uint8_t pal[12][4];                  /* 32: the palette of classes 1 .. 12: R, G, B and the blend weight a */
	uint8_t iso[4];                      /* 80 */
	uint32_t reserved[3];                /* 84 */
} smhv_ballistic_options;
typedef struct {
	uint32_t valid;                      /*  0 */
	uint32_t source_mask;                /*  4 */
	float origin[2];                     /*  8 */
	uint32_t count[12];                  /* 16: classes 1 .. 12 */
	uint32_t iso;                        /* 64 */
	uint32_t n_tof;                      /* 68 */
	double tof_min, tof_max;             /* 72, 80 */
	uint32_t reserved[2];                /* 88 */
} smhv_ballistic_map_result;             /* 96 bytes */
typedef struct {
	void *classes;                       /*  0: SMHV_BMAP_CLASSES: out_w * out_h bytes per frame, device memory */
	void *tof;                           /*  8: SMHV_BMAP_TOF: out_w * out_h floats per frame, device memory */
} smhv_ballistic_planes;                 /* 16 bytes */
#ifdef __cplusplus
static_assert(sizeof(smhv_weapon) == 80 && sizeof(smhv_weapon_rule) == 136 && sizeof(smhv_ballistic_arc) == 48 && sizeof(smhv_ballistic_solution) == 128,
              "ballistics layout");
static_assert(sizeof(smhv_ballistic) == 256 && sizeof(smhv_ballistic_options) == 96 && sizeof(smhv_ballistic_map_result) == 96, "ballistic map layout");
#endif
/* Host only, no device needed.  defaults: the reference's mortar -- velocity 109.890938, gravity 9.8, SMHV_ARC_HIGH, MILS6400, elev_min
 * 0, elev_max 1600 (a quarter turn: no limit), range_min 0, dispersion 0.  check: the list above.  thresholds: check, then the rule's
 * terms.  solve: thresholds, then the solution of (meters, alt) with source 0. */
SMHV_API int smhv_weapon_defaults(smhv_weapon *w);
SMHV_API int smhv_weapon_check(const smhv_weapon *w);
SMHV_API int smhv_weapon_thresholds(const smhv_weapon *w, smhv_weapon_rule *out);
SMHV_API int smhv_ballistic_solve(const smhv_weapon *w, double meters, double alt, smhv_ballistic_solution *out);
/* Host only.  Fills *opt: size, flags = PAINT, origin_mode = POINT at (0, 0), iso_s = 0 and the palette: out of range (200, 30, 30,
 * 96), below the minimum range (120, 120, 120, 96), mount too low (150, 60, 160, 96), mount too high (90, 60, 200, 96), the bands
 * smhv_reach_defaults' eight, iso (255, 255, 255, 160). */
SMHV_API int smhv_ballistic_defaults(smhv_ballistic_options *opt);
/* The weapon's solutions of the detected lines of frames [first, first + n), asynchronously on `stream`, into the batch's ballistics
 * slab (allocated by the first call): the records as after smhv_batch_run with SMHV_STAGE_MARKERS.  hm, fopt as smhv_batch_clearance
 * takes them.  SMHV_E_INVALID: what smhv_weapon_check and smhv_firing_solutions' options check refuse, n == 0, a range beyond the
 * batch's capacity, a heightmap on another device.  A failed call enqueues nothing. */
SMHV_API int smhv_batch_ballistics(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_firing_options *fopt,
                                   const smhv_weapon *weapon, void *stream);
SMHV_API int smhv_batch_read_ballistics(smhv_batch *b, uint32_t first, uint32_t n, smhv_ballistic_result *out);
SMHV_API int smhv_batch_ballistics_ptr(smhv_batch *b, void **d_ballistics);
/* The same for explicit lines, shaped like smhv_firing_solutions. */
SMHV_API int smhv_ballistic_lines(smhv_ctx *ctx, const smhv_line *lines, uint32_t n, const double *mpx, const uint32_t minimap[4], const smhv_heightmap *hm,
                                  const smhv_firing_options *fopt, const smhv_weapon *weapon, smhv_ballistic *out);
/* The ballistic map of frames [first, first + n), asynchronously on `stream`: smhv_batch_reach's contract (the results cleared ahead
 * of the kernels, PAINT behind the most recent render and SMHV_E_STATE before it or at another window, the heightmap's reference).
 * planes (NULL: none) names the planes' device memory, each starting at the call's first frame.  SMHV_E_INVALID: what
 * smhv_weapon_check refuses, a wrong size, unknown flags, an unknown origin_mode, line >= SMHV_MAX_LINES, an iso_s that is negative or
 * not finite, a plane flag without its pointer, what smhv_batch_render rejects in ropt, n == 0, a range
 * beyond the batch's capacity, a heightmap on another device.  A failed call enqueues nothing. */
SMHV_API int smhv_batch_ballistic_map(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *ropt,
                                      const smhv_weapon *weapon, const smhv_ballistic_options *opt, const smhv_ballistic_planes *planes, void *stream);
SMHV_API int smhv_batch_read_ballistic_map(smhv_batch *b, uint32_t first, uint32_t n, smhv_ballistic_map_result *out);
SMHV_API int smhv_batch_ballistic_map_ptr(smhv_batch *b, void **d_ballistic_map);
/* The per-call path, stateless like smhv_reach_map: origin_mode must be POINT; rgba_inout, classes (out_w * out_h bytes), tof (out_w *
 * out_h floats) and result may each be NULL, not all of them.  opt->flags is checked and otherwise not used. */
SMHV_API int smhv_ballistic_map(smhv_ctx *ctx, const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_weapon *weapon,
                                const smhv_ballistic_options *opt, const double *mpx, const uint32_t minimap[4], uint8_t *rgba_inout, uint8_t *classes,
                                float *tof, smhv_ballistic_map_result *result);

/* ---- ballistic clearance: a caller-supplied weapon's high and low arc against the terrain --------------------------------------------
 * "ballistics" reads the heightmap at the two end points of a line; "terrain clearance" looks at what lies between them, but for the
 * reference's mortar on its high arc alone.  This pass holds BOTH arcs of the caller's weapon against the terrain in one march: the
 * low arc is where terrain masking bites, and a weapon that can fire both wants to know which of them gets through.  The high arc
 * lies above the low arc everywhere between the ends (a_hi(x) - a_lo(x) = x (T_hi - T_lo)(1 - x / d) >= 0), so the answers of
 * interest are "the low arc is blocked, the high one clears" and "the high arc is beyond the mount's limit, the low one clears or not".
 * A verdict exists exactly where "terrain clearance" has one: the heightmap branch, all four rounded end-point coordinates inside the
 *   heightmap.  The end coordinates (x0, y0), (x1, y1), d, h0, h1, alt, S, the texel of sample k, the terrain z and the sight line
 *   l = alt * t are "terrain clearance"'s, word for word; d and alt are therefore bit-equal to smhv_ballistic_lines' meters and
 *   alt_delta on that branch.  What changes is the arc.  Every operation is ONE IEEE f64 operation, left to right, unfused.
 * Weapon terms, w = the weapon's smhv_weapon_rule ("ballistics": computed on the host once per call, never on the device):
 *   disc = w.v4 - w.g * (w.g * (d * d) + 2.0 * alt * w.v2);  s = sqrt(disc);  gm = w.g * d;  and for each arc a in {SMHV_ARC_HIGH,
 *   SMHV_ARC_LOW}:  T_a = (w.v2 + s) / gm (HIGH), (w.v2 - s) / gm (LOW);  qq1_a = 1.0 + T_a * T_a;  bal_a = "ballistics"' status bits
 *   of (disc, d, T_a) -- SMHV_BAL_OUT_OF_RANGE, _BELOW_MIN_RANGE, _ELEV_LOW, _ELEV_HIGH exactly as defined there.
 * Interior samples k = 1 .. S - 1:  t = (double)k / (double)S;  x = d * t;  per arc
 *   a_a = x * T_a - ((w.g * (x * x)) * qq1_a) / (2.0 * w.v2);  m_a = a_a - z;  the sample blocks arc a iff m_a < opt->margin_m.
 *   The sample blocks the sight line iff l < z.  With smhv_weapon_defaults this is "terrain clearance"'s expression on the high arc,
 *   operation for operation, on bit-equal constants.
 * Per arc (smhv_arc_clearance): status (SMHV_CLEAR_OUT_OF_RANGE / _CLEAR / _BLOCKED), first_blocked, n_blocked, min_margin, min_at are
 *   smhv_clearance_dir's fields by its rules: !(disc >= 0) is OUT_OF_RANGE with no arc (first_blocked = S, the rest 0); d == 0.0 is
 *   CLEAR with no samples; best starts at +inf and is replaced only when m < best (a NaN never wins, ties go to the lowest k);
 *   min_margin is 0 when nothing replaced best or S == 1, min_at 0 while nothing replaced it.  bal = bal_a.  The march never looks at
 *   bal: an arc beyond the mount's limit still gets its CLEAR or BLOCKED.
 * Per direction (smhv_ballistic_clearance_dir): arc[2]; meters = d; alt_delta = alt; los_blocked = the count (also on an OUT_OF_RANGE
 *   line, 0 when d == 0.0); valid = 1 iff a verdict exists -- otherwise the record is all zeros; choice = the arc to fire as 1 + a, or
 *   0: 1 + w.arc if that arc's status is CLEAR and its bal is 0, otherwise 1 + the other arc under the same condition, otherwise 0.
 *   Direction 1 is the rule on the line (P1, P0): end coordinates swapped, h0 := h1, alt := -alt.
 * Dense (the ballistic clearance map): origin and target per window pixel are "reach map"'s (origin_mode, line, origin, the "no
 *   origin" rule); the rule above, direction 0, gives one byte per pixel: bits 0..2 the class of the weapon's own arc (w.arc), bits
 *   3..5 the class of the other arc, SMHV_BCLR_LOS (0x80) wherever the byte is not 0 and some sample blocks the sight line (d != 0.0),
 *   bit 6 always 0.  The class of an arc, in order of precedence: 0 SMHV_BCLR_NONE no verdict; 1 _OUT_OF_RANGE !(disc >= 0);
 *   2 _UNUSABLE the arc's bal != 0; 4 _BLOCKED d != 0.0 and some sample blocks it; 3 _CLEAR otherwise.  A pixel is a SWITCH pixel iff
 *   its own class is 2 or 4 and the other arc's class is 3: fire the other arc.
 *   bytes   (SMHV_BCLR_BYTES) out_w * out_h per frame, tightly packed.
 *   margin  (SMHV_BCLR_MARGIN) f32 per pixel: (float) of the own arc's min_margin as the line record reports it (0 when nothing
 *           replaced best) where the own class is 3 or 4; NaN elsewhere.
 *   paint   (SMHV_BCLR_PAINT) "reach map"'s integer blend with pal[own class - 1], then on a switch pixel with switch_arc, then on a
 *           pixel with the LOS bit with los; a weight of 0 leaves the pixel as it is.
 *   summary one smhv_ballistic_clearance_map_result per frame, cleared on the stream ahead of the kernel: valid, origin as "reach
 *           map"; own[c - 1], other[c - 1] = window pixels whose own / other arc has class c = 1 .. 4; los_blocked = pixels with the
 *           LOS bit; switch_arc = switch pixels. */
#define SMHV_BCLR_PAINT 1u             /* smhv_ballistic_clearance_options.flags: tint the render slab (per call: implied by rgba_inout) */
#define SMHV_BCLR_BYTES 2u             /*   ... write the class bytes (per call: implied by bytes) */
#define SMHV_BCLR_MARGIN 4u            /*   ... write the margin plane (per call: implied by margin) */
#define SMHV_BCLR_NONE 0u              /* the class of an arc at a pixel */
#define SMHV_BCLR_OUT_OF_RANGE 1u
#define SMHV_BCLR_UNUSABLE 2u
#define SMHV_BCLR_CLEAR 3u
#define SMHV_BCLR_BLOCKED 4u
#define SMHV_BCLR_LOS 0x80u            /* the map's byte: | this */
typedef struct {
	uint32_t size;                       /*  0: sizeof(smhv_ballistic_clearance_options) == 80 */
	uint32_t flags;                      /*  4: SMHV_BCLR_PAINT | _BYTES | _MARGIN (the map only; 0: the summary alone) */
	uint32_t samples;                    /*  8: S, 1 .. SMHV_CLEAR_MAX_SAMPLES */
	uint32_t origin_mode;                /* 12: the map: SMHV_REACH_ORIGIN_* */
	uint32_t line;                       /* 16: the map, _LINE_P0 / _LINE_P1: which line of the record, < SMHV_MAX_LINES */
	uint32_t reserved0;                  /* 20: 0 */
	float origin[2];                     /* 24: the map, _POINT: the origin, map-ROI coordinates */
	double margin_m;                     /* 32: metres an arc must keep over the terrain; finite, >= 0 */
	uint8_t pal[4][4];                   /* 40: the palette of own classes 1 .. 4: R, G, B and the blend weight a */
	uint8_t switch_arc[4];               /* 56 */
	uint8_t los[4];                      /* 60 */
	uint32_t reserved[4];                /* 64: 0 */
} smhv_ballistic_clearance_options;
typedef struct {
	uint32_t status;                     /*  0: SMHV_CLEAR_OUT_OF_RANGE / _CLEAR / _BLOCKED */
	uint32_t first_blocked;              /*  4: the least k that blocks this arc; S when there is none */
	uint32_t n_blocked;                  /*  8 */
	uint32_t bal;                        /* 12: SMHV_BAL_* of this arc */
	double min_margin;                   /* 16 */
	uint32_t min_at;                     /* 24 */
	uint32_t reserved;                   /* 28 */
} smhv_arc_clearance;                    /* 32 bytes */
typedef struct {
	smhv_arc_clearance arc[2];           /*  0: [SMHV_ARC_HIGH], [SMHV_ARC_LOW] */
	double meters;                       /* 64: d */
	double alt_delta;                    /* 72: the target over the muzzle, as this direction sees it */
	uint32_t los_blocked;                /* 80: samples that block the sight line (a count) */
	uint32_t valid;                      /* 84: 1 iff a verdict exists; 0: the record is all zeros */
	uint32_t choice;                     /* 88: 1 + the arc to fire, 0: neither */
	uint32_t reserved;                   /* 92 */
} smhv_ballistic_clearance_dir;          /* 96 bytes */
typedef struct { smhv_ballistic_clearance_dir dir[2]; } smhv_ballistic_clearance;   /* 192 bytes: [0] from p0 at p1, [1] from p1 at p0 */
typedef struct {
	uint32_t n_lines, reserved[3];       /* == the record's n_lines; lines beyond it are zero */
	smhv_ballistic_clearance line[SMHV_MAX_LINES];   /* 16 */
} smhv_ballistic_clearance_result;
typedef struct {
	uint32_t valid;                      /*  0 */
	uint32_t reserved0;                  /*  4 */
	float origin[2];                     /*  8 */
	uint32_t own[4];                     /* 16: pixels whose own arc has class 1 .. 4 */
	uint32_t other[4];                   /* 32: ... whose other arc has */
	uint32_t los_blocked;                /* 48 */
	uint32_t switch_arc;                 /* 52 */
	uint32_t reserved[2];                /* 56 */
} smhv_ballistic_clearance_map_result;   /* 64 bytes */
typedef struct {
	void *bytes;                         /*  0: SMHV_BCLR_BYTES: out_w * out_h bytes per frame, device memory */
	void *margin;                        /*  8: SMHV_BCLR_MARGIN: out_w * out_h floats per frame, device memory */
} smhv_ballistic_clearance_planes;       /* 16 bytes */
#ifdef __cplusplus
static_assert(sizeof(smhv_ballistic_clearance_options) == 80 && sizeof(smhv_arc_clearance) == 32 && sizeof(smhv_ballistic_clearance_dir) == 96,
              "ballistic clearance layout");
static_assert(sizeof(smhv_ballistic_clearance) == 192 && sizeof(smhv_ballistic_clearance_result) == 16 + 192 * SMHV_MAX_LINES &&
              sizeof(smhv_ballistic_clearance_map_result) == 64 && sizeof(smhv_ballistic_clearance_planes) == 16, "ballistic clearance map layout");
#endif
/* Host only.  Fills *opt: size, flags = PAINT, samples = 64, origin_mode = POINT at (0, 0), margin_m = 0 and the palette -- out of
 * range, unusable and clear (0, 0, 0, 0), blocked (230, 40, 40, 110), switch_arc (240, 190, 40, 110), los (0, 0, 0, 70). */
SMHV_API int smhv_ballistic_clearance_defaults(smhv_ballistic_clearance_options *opt);
/* Host only, no device needed: what the entry points below refuse in opt (SMHV_E_INVALID), and nothing else. */
SMHV_API int smhv_ballistic_clearance_check(const smhv_ballistic_clearance_options *opt);
/* Both arcs of the weapon against the terrain, for the detected lines of frames [first, first + n), asynchronously on `stream`, into
 * the batch's ballistic-clearance slab (allocated by the first call): smhv_batch_clearance's contract with the weapon of
 * smhv_batch_ballistics.  Of opt, samples and margin_m apply (the rest is checked).  No elevation profile is written here;
 * smhv_batch_clearance gives one.  SMHV_E_INVALID: what smhv_weapon_check refuses, a wrong size, unknown flags, samples 0 or above
 * SMHV_CLEAR_MAX_SAMPLES, a margin_m that is negative or not finite, an unknown origin_mode, line >= SMHV_MAX_LINES with a line origin,
 * a reserved word that is not 0, what smhv_firing_solutions rejects in fopt, n == 0, a range beyond the batch's capacity, a heightmap on
 * another device.  A failed call enqueues nothing. */
SMHV_API int smhv_batch_ballistic_clearance(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_firing_options *fopt,
                                            const smhv_weapon *weapon, const smhv_ballistic_clearance_options *opt, void *stream);
SMHV_API int smhv_batch_read_ballistic_clearance(smhv_batch *b, uint32_t first, uint32_t n, smhv_ballistic_clearance_result *out);
SMHV_API int smhv_batch_ballistic_clearance_ptr(smhv_batch *b, void **d_ballistic_clearance);
/* The same for explicit lines, shaped like smhv_clearance_lines: out receives n records. */
SMHV_API int smhv_ballistic_clearance_lines(smhv_ctx *ctx, const smhv_line *lines, uint32_t n, const uint32_t minimap[4], const smhv_heightmap *hm,
                                            const smhv_firing_options *fopt, const smhv_weapon *weapon, const smhv_ballistic_clearance_options *opt,
                                            smhv_ballistic_clearance *out);
/* The ballistic clearance map of frames [first, first + n), asynchronously on `stream`: smhv_batch_clearance_map's contract (the
 * results cleared ahead of the kernel, PAINT behind the most recent render and SMHV_E_STATE before it or at another window, the
 * heightmap's reference) with the errors listed above.  planes (NULL: none) names the planes' device memory, each starting at the
 * call's first frame; a plane flag without its pointer is refused. */
SMHV_API int smhv_batch_ballistic_clearance_map(smhv_batch *b, uint32_t first, uint32_t n, const smhv_heightmap *hm, const smhv_render_options *ropt,
                                                const smhv_weapon *weapon, const smhv_ballistic_clearance_options *opt,
                                                const smhv_ballistic_clearance_planes *planes, void *stream);
SMHV_API int smhv_batch_read_ballistic_clearance_map(smhv_batch *b, uint32_t first, uint32_t n, smhv_ballistic_clearance_map_result *out);
SMHV_API int smhv_batch_ballistic_clearance_map_ptr(smhv_batch *b, void **d_ballistic_clearance_map);
/* The per-call path, stateless like smhv_clearance_map: origin_mode must be POINT; rgba_inout, bytes (out_w * out_h bytes), margin
 * (out_w * out_h floats) and result may each be NULL, not all of them.  opt->flags is checked and otherwise not used. */
SMHV_API int smhv_ballistic_clearance_map(smhv_ctx *ctx, const smhv_heightmap *hm, const smhv_render_options *ropt, const smhv_weapon *weapon,
                                          const smhv_ballistic_clearance_options *opt, const uint32_t minimap[4], uint8_t *rgba_inout, uint8_t *bytes,
                                          float *margin, smhv_ballistic_clearance_map_result *result);

#ifdef __cplusplus
}
#endif
#endif
