/* include/tfrec_amd.h -- C ABI of the MI355X-native IQ->telegram hot path.
 *
 * This is the drop-in boundary for baycom/tfrec's inner loop.  In the reference one receiver does, per
 * 65536-byte block of raw 8-bit IQ (engine.cpp:63-93):
 *
 *     datab[n] = (buf[n]-128)<<6;                      engine.cpp:77-78
 *     ld = dc.process_iq(data, len, filter_type);      engine.cpp:85   (dsp_stuff.cpp:243-264)
 *     fsk->process(data, ld);                          engine.cpp:86   (fm_demod.cpp:34-74)
 *         -> demodulator::start / ::demod              decoder.h:65-67 (tfa1.cpp:143, tfa2.cpp:346, whb.cpp:632)
 *         -> decoder::store_bit ... decoder::flush     decoder.h:39-40 (tfa1.cpp:120/47, tfa2.cpp:281/64, whb.cpp:566/477)
 *
 * Here the same work is done for a BATCH of independent streams on one GPU: tfrec_amd_submit_*()
 * replaces the three calls above for every stream of the batch, and tfrec_amd_drain_events() hands
 * back, per (stream, demodulator slot) and in order, what each reference decoder would have held at
 * the moment demodulator::demod() called decoder::flush(rssi, offset): byte_cnt, rdata[], the raw
 * RSSI accumulator and the frequency offset.  A host adapter replays each event into an (unchanged)
 * reference decoder object with decoder::store_bytes(ev.rdata, ev.byte_cnt) + decoder::flush(
 * tfrec_amd_rssi_db(...), ev.offset) -- the reference's own "-X" test entry (main.cpp:45-49,
 * decoder.cpp:35-40) -- see INTEGRATION.md.
 *
 * Plain C types only; caller-owned buffers; int return codes (0 = ok, <0 = TFREC_AMD_E_*); no
 * exceptions cross this boundary.  One host thread per context; contexts are independent (one per GPU
 * in a multi-GPU job: streams shard by index, no collective is involved).
 */
#ifndef TFREC_AMD_H
#define TFREC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFREC_AMD_BLOCK_BYTES 65536 /* RLS, engine.cpp:68 */
#define TFREC_AMD_FIFO_DEPTH 4  /* submits that may wait to be drained (tfrec_amd_drain_events); a property of the built
				   library: tfrec_amd_fifo_depth() reports the value it was compiled with */
#define TFREC_AMD_BLOCK_BYTES_10X 655360 /* one block of a 15.36 MS/s stream (TFREC_AMD_F_INPUT_10X) */
#define TFREC_AMD_BLOCK_DEC 8192    /* decimated IQ pairs per block (4:1, dsp_stuff.cpp:243-264) */
#define TFREC_AMD_NSLOTS 5

/* demodulator slots = registration order of main.cpp:173-218 */
enum { TFREC_AMD_SLOT_TFA1 = 0, TFREC_AMD_SLOT_TFA2 = 1, TFREC_AMD_SLOT_TFA3 = 2, TFREC_AMD_SLOT_TX22 = 3,
       TFREC_AMD_SLOT_WHB = 4 };

/* error codes */
enum {
	TFREC_AMD_OK = 0,
	TFREC_AMD_E_INVAL = -1,     /* bad argument / unsupported configuration */
	TFREC_AMD_E_NOMEM = -2,     /* host or device allocation failed */
	TFREC_AMD_E_HIP = -3,       /* a HIP runtime call failed (no device, launch failure, ...) */
	TFREC_AMD_E_OVERFLOW = -4,  /* event buffer too small: events were dropped */
	TFREC_AMD_E_STATE = -5      /* call sequence error */
};

/* config.flags */
#define TFREC_AMD_F_ALL_FLUSHES 1u /* emit an event for EVERY decoder::flush call (parity/debug mode); default:
				      only flushes whose byte_cnt reaches the decoder's minimum length
				      (tfa1.cpp:49, tfa2.cpp:76/222, whb.cpp:484) */
#define TFREC_AMD_F_TIMING 2u      /* record HIP events around every kernel (tfrec_amd_get_timings) */
#define TFREC_AMD_F_INPUT_10X 8u   /* BASELINE config 5: the input is u8 IQ at 15.36 MS/s (TFREC_AMD_BLOCK_BYTES_10X bytes per
				      block and stream); a 10:1 decimating FIR in the reference's integer style (60 int16
				      taps, >>16 per tap, int16 store; defined in DESIGN.md, no reference counterpart)
				      produces the 1.536 MS/s int16 stream that enters downconvert::process_iq */
#define TFREC_AMD_F_BITS 16u        /* parity/debug: besides the flush events, report every bit the demodulators hand to
				      decoder::store_bit (decoder.h:39; tfa1.cpp:120, tfa2.cpp:281, whb.cpp:566) as BITS events: status
				      = TFREC_AMD_STATUS_BITS, byte_cnt = bits in this chunk (<= 512), rdata = the bits, LSB first,
				      seq = ordinal of the flush they precede, end_sample = the first sample of their trigger window (counted like a
				      flush's), offset = the chunk's index: (end_sample, offset) is their order within that flush.
				      Window-parallel pipeline only. */
#define TFREC_AMD_F_LEVELS 32u       /* level meter: one tfrec_amd_level per stream and block of every submit (tfrec_amd_read_levels,
				      below).  A context without it launches exactly what it launched before */
#define TFREC_AMD_F_SERIAL_CHAINS 4u /* run the demodulators as one serial lane per (stream, slot) -- the simple
				      GPU formulation kept as a cross-check of the window-parallel pipeline */

typedef struct {
	int32_t n_streams;   /* independent IQ streams in the batch (>=1) */
	int32_t types_mask;  /* bit n = sensor_e n as main.cpp -T: TFA_1 0x01, TFA_2 0x02, TFA_3 0x04, TX22 0x08, WHB 0x20 */
	int32_t thresh;      /* trigger threshold, main.cpp -t; 0 = the reference's auto mode (starts at 500, adapts by +-2
				every 4th block, fm_demod.cpp:23-27, 58-73) */
	int32_t filter_type; /* 0 = narrow, 1 = wide (-W), dsp_stuff.cpp:176-178 */
	int32_t device;      /* HIP device ordinal */
	int32_t max_blocks;  /* largest n_blocks a submit may carry (sizes the device buffers) */
	int32_t max_events;  /* device event buffer capacity per submit/drain cycle */
	uint32_t flags;      /* TFREC_AMD_F_* */
} tfrec_amd_config;

#define TFREC_AMD_STATUS_BITS 0x80 /* event.status of a BITS chunk (TFREC_AMD_F_BITS) */

/* One decoder::flush() call site (tfa1.cpp:180, tfa2.cpp:434, whb.cpp:696).  96 bytes. */
typedef struct {
	uint32_t stream;    /* stream index within the batch */
	uint8_t slot;       /* TFREC_AMD_SLOT_* */
	uint8_t status;     /* 1 = passes the decoder's CRC + sanity checks (a telegram), 2 = rejected, 0 = shorter than a telegram */
	uint16_t byte_cnt;  /* decoder byte_cnt at flush (saturated at 65535) */
	int32_t offset;     /* second flush() argument (tfa2.cpp:434; 0 for TFA_1 and WHB) */
	uint32_t seq;       /* ordinal of this flush within (stream, slot) since context creation (or the stream's last reset) */
	int64_t end_sample; /* decimated sample index (since stream start or its last reset) at which flush fired */
	int64_t rssi_raw;   /* raw RSSI accumulator: tfa1.cpp:161, tfa2.cpp:373, whb.cpp:678 (an exact integer) */
	uint8_t rdata[64];  /* decoder rdata[0..64) at flush, before the decoder clears anything */
} tfrec_amd_event;

typedef struct tfrec_amd_ctx tfrec_amd_ctx;

/* kernel timings of the last submit (TFREC_AMD_F_TIMING), milliseconds */
typedef struct {
	float frontend_ms; /* (10:1 stage,) u8->s16 + 2-stage decimating FIR + trigger mask (+ auto-threshold pass) */
	float chains_ms;   /* all demodulator/decoder kernels together (end of front end -> end of last kernel) */
	float total_ms;    /* first kernel start to last kernel end */
	/* individual kernels of the window-parallel pipeline (0 when not run).  Window scan, then the TFA_2-family chain: */
	float windows_ms, spec_biquad_ms, repair_biquad_ms, fix_biquad_ms, slicer_ms, coop_slicer_ms, decode_ms, commit_ms;
	/* the WHB chain runs beside them on its own stream: its three biquad kernels together, then stage 2 */
	float whb_biquad_ms, whb_demod_ms, whb_decode_ms, whb_commit_ms; /* decode / commit: 0 (part of whb_demod) */
	/* ... and so does the TFA_1 chain (no biquad stage): short-window slicer, cooperative slicer, decode + commit */
	float tfa1_slicer_ms, tfa1_coop_slicer_ms, tfa1_decode_commit_ms;
	float fmdev_ms;    /* FM discriminator pass of the front end (tiles near trigger windows) */
	float whb_verify_ms; /* WHB stage 2 check: the exact decision-level recurrence, lane per stream (0: the exact stage 2 ran) */
} tfrec_amd_timings;

const char *tfrec_amd_version(void);
/* TFREC_AMD_FIFO_DEPTH of the loaded library (every submit in flight owns a full set of intermediate buffers: about
 * 7 GB per set and context at 1024 streams x 48 blocks -- several contexts on one device multiply that). */
int tfrec_amd_fifo_depth(void);
const char *tfrec_amd_strerror(int code);
/* text of the last HIP error seen by this thread ("" if none) */
const char *tfrec_amd_last_error(void);

/* Replaces, for cfg->n_streams receivers at once: `downconvert dc(2)` (engine.cpp:59), `fsk_demod fsk(&demods, thresh,
 * dbg)` (main.cpp:225) and the `new tfa1_demod / tfa2_demod / whb_demod` registrations of main.cpp:173-218
 * (types_mask = -T, thresh = -t, filter_type = -W). */
int tfrec_amd_create(const tfrec_amd_config *cfg, tfrec_amd_ctx **out);
int tfrec_amd_destroy(tfrec_amd_ctx *ctx);

/* Replaces n_blocks iterations of the block loop engine.cpp:67-86 for every stream: the u8 -> s16 conversion (:77-78),
 * downconvert::process_iq (:85, dsp_stuff.cpp:243-264) and fsk_demod::process (:86, fm_demod.cpp:34-74) with every
 * demodulator::start / ::demod and decoder::store_bit it drives (tfa1.cpp:120-190, tfa2.cpp:281-442, whb.cpp:566-707).
 * Process n_blocks 65536-byte blocks of every stream.  Stream s starts at d_iq + s*stream_stride_bytes
 * (device memory, u8 interleaved I,Q as the reference's -S dump files, sdr.cpp:233-234).  Asynchronous:
 * the work is ordered after what is already queued on hip_stream (a hipStream_t, NULL = default stream) -- the
 * producer of d_iq -- and runs on the context's own streams; d_iq must stay valid until the submit has been
 * drained (or tfrec_amd_sync returned).  All demodulator/decoder state carries over to the next submit exactly as
 * it carries from block to block in the reference.
 * A HIP failure in the middle of a submit (TFREC_AMD_E_HIP after work was enqueued) poisons the context: kernels may
 * already have advanced the carried state, so every later submit / drain returns TFREC_AMD_E_STATE until the context is
 * destroyed and recreated.  Argument errors (E_INVAL, a full FIFO) leave it untouched. */
int tfrec_amd_submit_device(tfrec_amd_ctx *ctx, const void *d_iq, size_t stream_stride_bytes, int n_blocks,
			    void *hip_stream);
/* Same with host memory: stages the batch through an internal device buffer (H2D copy included).  With pinned
 * memory (tfrec_amd_host_alloc) the copy is asynchronous and h_iq must stay untouched until the submit has been
 * drained; together with the submit/drain FIFO below this is the double-buffered feeder of SURVEY row f1: read batch
 * k+2 from disk while batch k+1 is copied/processed and batch k's events are dispatched. */
int tfrec_amd_submit_host(tfrec_amd_ctx *ctx, const uint8_t *h_iq, size_t stream_stride_bytes, int n_blocks);
/* Page-locked host memory for tfrec_amd_submit_host (NULL on failure). */
void *tfrec_amd_host_alloc(size_t bytes);
void tfrec_amd_host_free(void *p);

/* Mark streams[0..n) to restart as fresh receivers at the start of the NEXT submit -- what replugging or retuning one stick
 * of the reference means: restarting that one tfrec process.  Every other stream carries on untouched.
 *   - The reset falls between the last submit already queued and the next one.  Events of submits still in the FIFO are
 *     drained unchanged (old seq, old end_sample).  Calls made before one submit accumulate; duplicate indices are allowed;
 *     n == 0 is a no-op.
 *   - From the next submit on, a reset stream's events are exactly those of a fresh receiver (tfrec_amd_create with the
 *     stream's own current types_mask, thresh and filter_type -- the context's, unless tfrec_amd_configure_streams changed
 *     them -- and the context's flags) fed only the input that follows: seq restarts at 0 per slot and end_sample counts
 *     from the first sample after the reset.
 *   - A trigger window open at the reset point is dropped without a flush, as the reference drops it at the end of a dump
 *     (the process exits, engine.cpp:72-76): the events before the reset are those of a fresh receiver run on the old
 *     input truncated at the cut.
 *   - Auto threshold (thresh == 0): the stream restarts at 500 (fm_demod.cpp:23-27); tfrec_amd_read_thresh shows it once
 *     the next submit has run.
 *   - Context-wide counters (tfrec_amd_get_stats, tfrec_amd_get_fm_stats, timings) are not reset.
 *   - Every mode: both pipeline layouts, TFREC_AMD_F_SERIAL_CHAINS, _INPUT_10X, _BITS, _ALL_FLUSHES.
 *   - Cost: a submit that carries resets starts its front end only once every stage of the submit before it has ended (it
 *     does not overlap it: about twice the period at the benchmark size, however few streams it resets); a
 *     submit without one runs exactly as before.
 * Errors: an index outside [0, n_streams), n < 0, or streams == NULL with n > 0: TFREC_AMD_E_INVAL, and nothing is
 * marked.  A poisoned context: TFREC_AMD_E_STATE. */
int tfrec_amd_reset_streams(tfrec_amd_ctx *ctx, const int32_t *streams, int n);

/* Settings of one stream: what -T, -t and -W are to one tfrec process of the reference. */
typedef struct {
	int32_t types_mask;  /* demodulators of this stream: a non-empty subset of the context's types_mask */
	int32_t thresh;      /* trigger threshold >= 0; 0 = the reference's auto mode, starting at 500 */
	int32_t filter_type; /* 0 narrow, 1 wide (-W) */
	int32_t reserved;    /* must be 0 */
} tfrec_amd_stream_config;

/* Give streams[i] the settings cfgs[i] (i < n), as a fresh receiver from the NEXT submit on.  The context's types_mask is the
 * set of demodulators it builds; its thresh and filter_type are every stream's initial settings.
 *   - The restart is exactly that of tfrec_amd_reset_streams (the same cut, the dropped open window, seq and end_sample
 *     restarting, other streams untouched), but the stream comes back with its new settings.  A later reset keeps them.
 *   - Before the first submit this only sets the settings.  Duplicate indices are allowed: the last one wins.  A reset and a
 *     configure of one stream before one submit are one restart, with the latest settings.  n == 0 is a no-op.
 *   - Flags stay context-wide (TFREC_AMD_F_BITS, _ALL_FLUSHES, _INPUT_10X, _SERIAL_CHAINS, _TIMING).
 *   - A context in which no stream was ever configured runs exactly as before.  Cost: that of a reset.
 * Errors: an index outside [0, n_streams), n < 0, streams or cfgs NULL with n > 0, a types_mask that is empty or names a
 * demodulator outside the context's types_mask, thresh < 0, filter_type not 0 or 1, reserved != 0: TFREC_AMD_E_INVAL, and
 * nothing is marked.  A poisoned context: TFREC_AMD_E_STATE. */
int tfrec_amd_configure_streams(tfrec_amd_ctx *ctx, const int32_t *streams, const tfrec_amd_stream_config *cfgs, int n);
/* The settings the next submit will use for one stream. */
int tfrec_amd_get_stream_config(tfrec_amd_ctx *ctx, int stream, tfrec_amd_stream_config *out);

/* Tune streams[i] to tune_hz[i] (i < n): what -f, the receive frequency, is to one tfrec process of the reference, applied to
 * recorded IQ.  tune_hz is the offset of the wanted channel from the centre of the recording (f - f_recorded, in Hz), and
 * |tune_hz| < 768000.  No reference counterpart: the stage is defined here and pinned by a CPU restatement
 * (tfrec_amd/tune.py).  It acts on the 1.536 MS/s int16 (I, Q) stream that enters downconvert::process_iq -- the default
 * input x = (u8 - 128) << 6, with TFREC_AMD_F_INPUT_10X the output of the 10:1 stage:
 *     inc  = floor((tune_hz * 2^33 + 1536000) / 3072000) mod 2^32       (exact 64-bit integers, floor division)
 *     p    = (n * inc) mod 2^32,  k = p >> 20                          (n: the sample's index since the stream's start or
 *                                                                        last restart; the FIR history before it is silence)
 *     C[k] = round(32767 * cos(2 pi k / 4096)),  S[k] = C[(k - 1024) mod 4096]
 *     I'   = sat16((I * C[k] + Q * S[k] + 2^14) >> 15),  Q' = sat16((Q * C[k] - I * S[k] + 2^14) >> 15)   (int32, arithmetic >>)
 * A signal at +tune_hz in the recording is moved to DC.  tune_hz = 0 means no mixing: the stream is bit for bit what it is
 * untuned.  The rest of the path is the reference's process_iq on int16 input.
 *   - A tune is a restart with exactly the semantics of tfrec_amd_configure_streams: the same cut and dropped open window,
 *     seq and end_sample restarting, other streams untouched.  Before the first submit it only sets the value.  Duplicate
 *     indices: the last one wins.  A reset, a configure and a tune of one stream before one submit are one restart with the
 *     latest values; later resets and configures keep the tune.  n == 0 is a no-op.
 *   - A context in which no stream has a tune other than 0 launches the kernels of an untuned context.  Cost: that of a reset
 *     for the restart, and the rotation in the front end while a stream is tuned.
 * Errors: an index outside [0, n_streams), n < 0, streams or tune_hz NULL with n > 0, |tune_hz| >= 768000:
 * TFREC_AMD_E_INVAL, and nothing is marked.  A poisoned context: TFREC_AMD_E_STATE. */
int tfrec_amd_tune_streams(tfrec_amd_ctx *ctx, const int32_t *streams, const int32_t *tune_hz, int n);
/* The tune the next submit will use for one stream (0: untuned). */
int tfrec_amd_get_stream_tune(tfrec_amd_ctx *ctx, int stream, int32_t *tune_hz);

/* Shared inputs: stream streams[i] reads input row inputs[i] (0 <= inputs[i] < n_streams) from the NEXT submit on:
 * its samples start at iq + inputs[i] * stream_stride_bytes.  Default: the identity (stream s reads row s).  Several streams may
 * read one row: K receivers of one wide recording (each with its own tune and settings) need the recording in the batch once.
 *   - A map is a restart with exactly the semantics of tfrec_amd_configure_streams / tfrec_amd_tune_streams: the same cut and
 *     dropped open window, seq and end_sample restarting, other streams untouched.  Before the first submit it only sets the
 *     value.  Duplicate indices: the last one wins.  A reset, configure, tune and map of one stream before one submit are ONE
 *     restart with the latest values; later resets keep the map.  Mapping a stream to the row it reads already is still a
 *     restart.  n == 0 is a no-op.
 *   - Only the address a stream's samples are loaded from changes.  Everything a receiver carries stays its own, the FIR
 *     history included: two streams on one row that restarted at different times have different histories.
 *   - A submit must provide rows 0 .. R-1, R = 1 + the highest row a stream reads.  tfrec_amd_submit_device reads only those;
 *     tfrec_amd_submit_host stages and copies only those (this is the saving: K receivers of one row cost one row of PCIe).
 *     The stride rules of the submits are unchanged.
 *   - A context in which no stream was ever mapped launches the kernels it launched before.  A mapped context of the default
 *     input runs the per-stream tuned front end (the cost of tfrec_amd_tune_streams); with
 *     TFREC_AMD_F_INPUT_10X the 10:1 stage's tuned kernel looks the row up and the front end is unchanged.
 * Errors: a stream index or an input outside [0, n_streams), n < 0, streams or inputs NULL with n > 0: TFREC_AMD_E_INVAL, and
 * nothing is marked.  A poisoned context: TFREC_AMD_E_STATE. */
int tfrec_amd_map_streams(tfrec_amd_ctx *ctx, const int32_t *streams, const int32_t *inputs, int n);
/* The input row the next submit will read for one stream. */
int tfrec_amd_get_stream_input(tfrec_amd_ctx *ctx, int stream, int32_t *input);

/* Wideband tune (TFREC_AMD_F_INPUT_10X contexts only): a frequency shift AHEAD of the 10:1 stage, so that a
 * receiver can sit anywhere in the 15.36 MS/s input.  |tune_hz| < 7680000.  It is tfrec_amd_tune_streams' mixer at the input
 * rate, on the int16 stream x = (u8 - 128) << 6 the 10:1 stage is defined on (same table C, S and the same rounding):
 *     inc10 = floor((tune_hz * 2^33 + 15360000) / 30720000) mod 2^32
 *     p     = (n * inc10) mod 2^32,  k = p >> 20        (n: the INPUT sample's index since the stream's start or last restart;
 *                                                         the history before a restart is silence)
 *     I'    = sat16((I * C[k] + Q * S[k] + 2^14) >> 15),  Q' = sat16((Q * C[k] - I * S[k] + 2^14) >> 15)
 *     y0[m] = int16( sum_{n<60} ( x'[10 m - 50 + n] * h10[n] ) >> 16 )                           (the 10:1 stage, unchanged)
 * tune_hz = 0 is no mixing: bit for bit the stage as it is.  tfrec_amd_tune_streams composes: it acts on y0.
 * tfrec_amd_read_stage0 returns the shifted, decimated y0.  Pinned by tfrec_amd/tune.py (inc10, mix10_s16, decim10_s16).
 *   - A wide tune is a restart, with the semantics, the "last wins" and the composition rules of tfrec_amd_map_streams.
 *   - A context without a wide tune and without a map launches the 10:1 kernel it launched before.
 * Errors: as tfrec_amd_tune_streams with the limit above; a context without TFREC_AMD_F_INPUT_10X: TFREC_AMD_E_INVAL. */
int tfrec_amd_tune_streams_wide(tfrec_amd_ctx *ctx, const int32_t *streams, const int32_t *tune_hz, int n);
/* The wide tune the next submit will use for one stream (0: none). */
int tfrec_amd_get_stream_tune_wide(tfrec_amd_ctx *ctx, int stream, int32_t *tune_hz);

/* Other input rates: a context for u8 IQ at fs_in = 1536000 * rate_p / rate_q samples per second -- 2.048 MS/s is
 * 4/3, 2.4 MS/s 25/16, 1.92 MS/s 5/4 -- which a resampling stage on the GPU brings to the 1.536 MS/s int16 (I, Q) stream that
 * enters downconvert::process_iq; the rest of the path is unchanged.  No reference counterpart: like the 10:1 stage and the
 * tuners the stage is defined here, in the reference's FIR style, and pinned by a CPU restatement (tfrec_amd/resample.py).
 *   Rates:   gcd(P, Q) = 1, 1 < P/Q < 10, and Q <= 64 or Q divides 1536.  r = P/Q is the number of input samples per output sample.
 *            "Q divides 1536" is "fs_in is a whole number of kHz": every whole-kHz rate with 1536000 < fs_in < 15360000 is accepted
 *            -- 2.0 MS/s is 125/96, 2.5 MS/s 625/384, 5 MS/s 625/192, 10 MS/s 625/96, 12.5 MS/s 3125/384.  Other denominators
 *            above 64 (97/80, 1025/1024), rates up to 1.536 MS/s and from 15.36 MS/s on are refused.
 *   Filter:  T = 2 * ceil(3 r) taps per phase (even, <= 60; 8 at 2.048 MS/s, 10 at 2.4 MS/s).  For output sample m, counted since
 *            the stream's start or last restart:  a = m P,  i0 = floor(a / Q),  phi = a mod Q   (exact 64-bit integers)
 *   Output:  y0[m] = int16( sum_{n<T} ( x[i0 - (T-1) + n] * h[phi][n] ) >> 16 )   per rail, int32 arithmetic, arithmetic shifts,
 *            x = (u8 - 128) << 6, x[<0] = 0 (the history before a start or restart is silence, u8 128).  Causal: the newest
 *            sample used is i0, so a submit never reads past its own input.
 *   Taps:    d = n - T/2 + 1 - phi/Q  (in (-T/2, T/2]),  g = sinc(d / r) (0.54 + 0.46 cos(2 pi d / T)),  sinc(u) = sin(pi u)/(pi u),
 *            sinc(0) = 1;  v = g * 65536 / sum_n g;  h[phi][n] = round(v); the residual 65536 - sum_n h is added to the tap with
 *            the largest v (the lowest n among equals): every phase sums to exactly 65536, unity DC gain as for the 10:1 taps.
 *            Computed in double.  (A tap reaches about 65536 / r: the table is int32, not int16.)
 *   Refused: a rate where any v lies within 1e-9 of a rounding tie (the table must not depend on the host's libm), or where
 *            max_phi sum_n |h[phi][n]| * 8192 >> 16 >= 32768 (so the int16 store never wraps for u8 input): TFREC_AMD_E_INVAL.
 *   Submits: n_blocks blocks (TFREC_AMD_BLOCK_DEC decimated samples each, as always) consume exactly
 *            n_in = n_blocks * 32768 * P / Q complex input samples per stream, n_in * 2 bytes per input row; n_blocks must be a
 *            multiple of unit(Q) = Q / gcd(Q, 64) -- the odd part of a Q <= 64, so any value when that Q is a power of two; 3, 2,
 *            3, 4, 6, 8, 12, 24 at Q = 96, 128, 192, 256, 384, 512, 768, 1536 --, or the submit returns TFREC_AMD_E_INVAL and
 *            nothing is queued.  Then n_in = k * P * 512 * (64 / gcd(Q, 64)) for a whole k: a whole number and a multiple of 512.
 *            (The odd part alone would not do above 64: one block of 129/128 is 33024 samples, 64.5 times 512.)  Every submit
 *            therefore begins at phase 0 on its own first input sample, and results do not depend on how a stream is cut into
 *            submits.  A context whose max_blocks is below unit(Q) can be made and takes no submit.
 * cfg->flags must not contain TFREC_AMD_F_INPUT_10X (TFREC_AMD_E_INVAL).  On such a context tfrec_amd_submit_device / _host take
 * n_in * 2 bytes per row (submit_host stages exactly that, rows 0 .. R-1), tfrec_amd_read_stage0 returns y0, tfrec_amd_get_memory
 * counts the stage's buffers, tfrec_amd_tune_streams_wide returns TFREC_AMD_E_INVAL (the tune ahead of this stage is
 * tfrec_amd_tune_streams_input, below), and everything else keeps its meaning, because nothing behind stage 0 changes: reset, configure, tune (it acts on y0)
 * and map (the stage looks the row up), both pipeline layouts, _SERIAL_CHAINS, _BITS, _ALL_FLUSHES, _TIMING.  A context made by
 * tfrec_amd_create launches the kernels it launched before. */
int tfrec_amd_create_rate(const tfrec_amd_config *cfg, int32_t rate_p, int32_t rate_q, tfrec_amd_ctx **out);
/* Input-rate tune: a frequency shift at the context's input rate fs_in = 1536000 * P / Q (what
 * tfrec_amd_get_input_rate reports), AHEAD of the resampling stage, so that a receiver can sit anywhere in a recording made at
 * that rate -- not only within the +-768 kHz that tfrec_amd_tune_streams, which acts behind the stage, can reach.  It is
 * tfrec_amd_tune_streams' mixer at the input rate, on x = (u8 - 128) << 6 (same table C, S and the same rounding):
 *     inc_in = floor((tune_hz * 2^33 * Q + 1536000 * P) / (2 * 1536000 * P)) mod 2^32          (exact integers, floor division)
 *     p      = (n * inc_in) mod 2^32,  k = p >> 20      (n: the INPUT sample's index since the stream's start or last restart)
 *     I'     = sat16((I * C[k] + Q * S[k] + 2^14) >> 15),  Q' = sat16((Q * C[k] - I * S[k] + 2^14) >> 15)
 *     y0[m]  = int16( sum_{n<T} ( x'[i0 - (T-1) + n] * h[phi][n] ) >> 16 )                  (the resampling stage, unchanged)
 * Limit: 2 * |tune_hz| * Q < 1536000 * P, that is |tune_hz| < fs_in / 2, tested in integers (the numerator of inc_in leaves 63
 * bits once |tune_hz| * Q >= 2^30 -- from 699051 Hz on at Q = 1536 -- and is computed in 128-bit integers).  With P/Q = 10/1 the formula is inc10, with 1/1 tfrec_amd_tune_streams' inc: one definition
 * for every rate.  tune_hz = 0 is no mixing: bit for bit the stage as it is.  The history before a start or restart is silence; a
 * history sample from the previous submit is rotated with its own (earlier) n.  The phase of a submit's first input sample is
 * (n0 * inc_in) mod 2^32, n0 = 4 * (decimated samples since the stream's origin) * P / Q, whole because every submit is.
 * tfrec_amd_tune_streams composes: it acts on y0.  tfrec_amd_read_stage0 returns the shifted, resampled y0.  Pinned by
 * tfrec_amd/tune.py (inc_in, mix_in_s16) and tfrec_amd/resample.py (resample_x16).
 *   No wrap: the mixer's output of u8 input is at most 11585 per rail, and the largest max_phi sum_n |h| of any accepted rate is
 *   108260 (at 769/768 and 1537/1536; 108112 at 65/64 is the largest with Q <= 64), so |y0| <= 108260 * 11585 >> 16 = 19137.  A
 *   guard stays: on a rate where
 *   max_phi sum_n |h[phi][n]| * 11585 >> 16 >= 32768 the call returns TFREC_AMD_E_INVAL.
 *   - An input tune is a restart, with the semantics, the "last wins" and the composition rules of tfrec_amd_map_streams /
 *     tfrec_amd_tune_streams_wide: reset + configure + tune + map + input tune before one submit are ONE restart; later resets
 *     keep the tune.
 *   - A context in which no stream has an input tune launches the kernels it launched before, and holds no more memory with one.
 *   - A TFREC_AMD_F_INPUT_10X context: the call IS tfrec_amd_tune_streams_wide (the same state; both getters return the same value).
 *     A context of the default input: TFREC_AMD_E_INVAL (its tune is tfrec_amd_tune_streams).
 * Errors: as tfrec_amd_tune_streams_wide, with the limit above. */
int tfrec_amd_tune_streams_input(tfrec_amd_ctx *ctx, const int32_t *streams, const int32_t *tune_hz, int n);
/* The input-rate tune the next submit will use for one stream (0: none). */
int tfrec_amd_get_stream_tune_input(tfrec_amd_ctx *ctx, int stream, int32_t *tune_hz);
/* The context's input rate as P/Q of 1.536 MS/s: 1/1 for tfrec_amd_create, 10/1 with TFREC_AMD_F_INPUT_10X. */
int tfrec_amd_get_input_rate(tfrec_amd_ctx *ctx, int32_t *p, int32_t *q);
/* Bytes one input row of a submit of n_blocks blocks holds (every kind of context); TFREC_AMD_E_INVAL when n_blocks < 1 or
 * is no multiple of unit(Q) (Submits, above). */
int tfrec_amd_input_bytes(tfrec_amd_ctx *ctx, int n_blocks, size_t *bytes_per_stream);
/* The tap table of a rate: taps[phi * T + n], Q * T values (cap: the room in `taps`, in values), T to *n_taps_per_phase.  taps may
 * be NULL with cap 0 (only T, or only the verdict, is wanted).  Needs no context and no GPU.  TFREC_AMD_E_INVAL: a rate outside
 * the rules above or refused by them, or cap too small. */
int tfrec_amd_resample_taps(int32_t rate_p, int32_t rate_q, int32_t *taps, int cap, int *n_taps_per_phase);
/* Sample formats: a context whose input rows are not the RTL-SDR's offset-binary u8 but what other recorders write --
 * signed int8 (hackrf_transfer), int16 (Airspy, SDRplay, USRP, rx_sdr) or float32 (GNU Radio, SDR++, GQRX, SigMF cf32_le) --, at
 * any rate tfrec_amd_create_rate accepts or at the base rate 1/1 (1.536 MS/s).  A format maps one stored component (I or Q,
 * little-endian, interleaved I, Q) to x, the int16 value every stage is defined on, -8192 <= x <= 8191; full scale maps to full
 * scale, so the trigger threshold and the auto threshold keep their meaning:
 *     format                bytes per complex sample   x
 *     TFREC_AMD_FMT_U8  0   2                          (u8 - 128) << 6   (as always)
 *     TFREC_AMD_FMT_S8  1   2                          s8 << 6           (the u8 value of byte ^ 0x80)
 *     TFREC_AMD_FMT_S16 2   4                          s16 >> 2, arithmetic shift
 *     TFREC_AMD_FMT_F32 3   8                          v = f * 8192 in fp32 (exact unless it overflows); x = clamp(rint(v), -8192, 8191),
 *                                                      rint ties to even; NaN gives 0; +-inf and overflow clamp
 * Everything after x is the text above: the input-rate tune's mixer acts on x at the input rate, the resampling stage
 * y0[m] = int16( sum_{n<T} ( x'[i0 - (T-1) + n] * h[phi][n] ) >> 16 ) follows, then tfrec_amd_tune_streams and process_iq on int16
 * input.  The history before a start or restart is x = 0.  The no-wrap arguments of the resampling stage and of the input-rate
 * tune hold unchanged, because |x| <= 8192 as for u8.  At 1/1 no resampler runs and no delay is introduced: stage 0 is x itself,
 * and an S8 context on bytes ^ 0x80 equals a tfrec_amd_create context on the bytes, bit for bit.  Pinned by tfrec_amd/formats.py
 * (to_x) ahead of resample.py (resample_x16) and tune.py (mix_in_s16).
 *   - TFREC_AMD_FMT_U8 IS tfrec_amd_create_rate, or tfrec_amd_create at 1/1: the same kernels, memory and behaviour.
 *   - Refused with TFREC_AMD_E_INVAL: an unknown format; TFREC_AMD_F_INPUT_10X with a format other than U8; a rate that is neither
 *     1/1 nor accepted by tfrec_amd_create_rate.
 *   - Rows: tfrec_amd_input_bytes returns n_in * bytes per complex sample, and tfrec_amd_submit_device / _host take that many bytes
 *     per row (submit_host's staging buffer grows with it).  The 16-byte alignment rules for base and stride are unchanged -- n_in
 *     is a multiple of 512 for every permitted submit, so every row size is a 16-byte multiple --, and so is the block-count rule.
 *   - Everything that works on a rate context works: reset, configure, tfrec_amd_tune_streams, tfrec_amd_map_streams,
 *     tfrec_amd_tune_streams_input, both layouts, _SERIAL_CHAINS, _BITS, _ALL_FLUSHES, _TIMING; tfrec_amd_read_stage0 returns y0 (at
 *     1/1: x); tfrec_amd_get_memory counts what the context holds.  At 1/1 the input-rate tune returns TFREC_AMD_E_INVAL, as on a
 *     tfrec_amd_create context (the tune there is tfrec_amd_tune_streams); tfrec_amd_tune_streams_wide returns TFREC_AMD_E_INVAL, as
 *     on any rate context.
 * Contexts made by tfrec_amd_create, tfrec_amd_create_rate or with TFREC_AMD_F_INPUT_10X launch the kernels they launched before. */
enum { TFREC_AMD_FMT_U8 = 0, TFREC_AMD_FMT_S8 = 1, TFREC_AMD_FMT_S16 = 2, TFREC_AMD_FMT_F32 = 3 };
int tfrec_amd_create_format(const tfrec_amd_config *cfg, int32_t format, int32_t rate_p, int32_t rate_q, tfrec_amd_ctx **out);
/* The context's input format (TFREC_AMD_FMT_U8 for every context of the older constructors). */
int tfrec_amd_get_input_format(tfrec_amd_ctx *ctx, int32_t *format);
/* DC blocker: a context that removes each input ROW's DC offset -- the constant a zero-IF front end adds to I and to
 * Q -- ahead of everything else.  It belongs to an input row, as the spectrum does, not to a stream: a row is corrected once, however
 * many streams read it.  It acts on x, the int16 value every format maps a stored component to (tfrec_amd_create_format), at the
 * context's input rate, ahead of the input-rate tune, the resampling stage, tfrec_amd_tune_streams and process_iq.  Exact integers:
 *   Windows.  L = 512 complex input samples; window w of a row covers its samples [512 w, 512 (w + 1)), counted from the row's first
 *     submit or its last DC reset.  Every permitted submit holds n_in = n_blocks * 32768 * P / Q samples, a multiple of 512: n_blocks
 *     is a multiple of Q / gcd(Q, 64), so n_in = k * P * 512 * (64 / gcd(Q, 64)) (tfrec_amd_create_rate: Submits).  So no window straddles a
 *     submit, and results do not depend on how a row is cut into submits.
 *   Sums.  S_I[w], S_Q[w] = the window's sums of x_I and x_Q (|S| <= 2^22).
 *   Estimate.  K = avg_windows, 1 <= K <= 4096; lo = max(0, w - K + 1), c = w - lo + 1, A = S[lo] + ... + S[w] per rail (window w's
 *     own sum included: a row's first window is already corrected), and
 *         d[w] = floor((2 A + 512 c) / (1024 c))
 *     in 64-bit integers -- floor, not C's truncation, for a negative numerator: the mean of the last c windows rounded half up.
 *     |2 A| < 2^36 and -8192 <= d <= 8191.
 *   Apply.  x' = clamp(x - d[w], -8192, 8191) per rail.  Everything downstream is the text above applied to x'; its no-wrap arguments
 *     hold because |x'| <= 8192.  The pre-stage's history after a stream restart stays x = 0.
 *   State.  Per row the last K window sums and the window count, carried from submit to submit.  A stream restart (reset, configure,
 *     tune, map, input tune) does not touch it; tfrec_amd_reset_dc_rows clears it at the next submit; a row that a submit does not
 *     provide (rows at or beyond the submit's rows in use) keeps it.
 * tfrec_amd_create_dc: `format` is any of the four, the rate 1/1 or any rate tfrec_amd_create_rate accepts; max_rows within
 * [1, n_streams] is the most input rows a submit may use (n_streams, or 1 + the highest row mapped): a submit that uses more returns
 * TFREC_AMD_E_INVAL and queues nothing.  TFREC_AMD_F_INPUT_10X is refused with TFREC_AMD_E_INVAL (no DC removal ahead of the 10:1
 * stage), as are avg_windows or max_rows outside their ranges, an unknown format and a rate the older constructors refuse.  The
 * context is a format context in every other respect: tfrec_amd_get_input_format, tfrec_amd_input_bytes, the submits and the
 * spectrum (which keeps reading the caller's raw rows: it shows the offset) see the caller's format; reset, configure, the tunes,
 * map, levels, capture, spectrum, occupancy, both layouts, _SERIAL_CHAINS, _BITS, _ALL_FLUSHES and _TIMING work; and
 * tfrec_amd_read_stage0 returns the stage-0 samples of the CORRECTED input.  Memory (all in tfrec_amd_get_memory): per FIFO set the
 * corrected rows, max_rows * n_max * 4 bytes (n_max: the largest submit's samples per row), and the table of d, 4 bytes per window;
 * per context the ring of sums (max_rows * K * 8 bytes), a submit's sums and the counts.  Pinned by tfrec_amd/dcblock.py.
 * Contexts of the older constructors launch what they launched before. */
int tfrec_amd_create_dc(const tfrec_amd_config *cfg, int32_t format, int32_t rate_p, int32_t rate_q, int32_t avg_windows, int32_t max_rows,
			tfrec_amd_ctx **out);
/* avg_windows and max_rows of a tfrec_amd_create_dc context; 0 and 0 on every other context. */
int tfrec_amd_get_dc(tfrec_amd_ctx *ctx, int32_t *avg_windows, int32_t *max_rows);
/* d[w] of one input row of the OLDEST undrained submit, with the conventions of tfrec_amd_read_levels (waits for the submit; call it
 * BEFORE tfrec_amd_drain_events pops it; reading pops nothing): d[2 * w] = the I rail's and d[2 * w + 1] = the Q rail's value of the
 * submit's window w, for w < *n_windows = n_in / 512; cap_windows is the room in windows.  d may be NULL with cap_windows 0 to fetch
 * only *n_windows.
 * Errors: not a tfrec_amd_create_dc context, a row the submit did not use, n_windows NULL: TFREC_AMD_E_INVAL; the room too small
 * (or d NULL): TFREC_AMD_E_INVAL, nothing is written, but *n_windows is set; nothing undrained or a poisoned context:
 * TFREC_AMD_E_STATE. */
int tfrec_amd_read_dc(tfrec_amd_ctx *ctx, int32_t row, int16_t *d, size_t cap_windows, int *n_windows);
/* Clear the DC state of the listed rows (each within [0, max_rows); duplicates allowed; n == 0: nothing) at the NEXT submit: their
 * window count restarts at 0 there.  Submits already queued are not affected; the streams that read the rows are not restarted.
 * Errors as tfrec_amd_reset_streams: a NULL list with n > 0, n < 0, a row out of range or a context without the blocker:
 * TFREC_AMD_E_INVAL, and nothing is marked; a poisoned context: TFREC_AMD_E_STATE. */
int tfrec_amd_reset_dc_rows(tfrec_amd_ctx *ctx, const int32_t *rows, int n);
/* IQ balancer: a context that removes each input ROW's IQ imbalance -- the gain and phase error between the I and
 * the Q rail of a zero-IF front end, which puts a conjugate image of every signal at the mirror frequency -- behind the DC blocker
 * (or without one) and ahead of everything else.  It belongs to an input row and acts at the context's input rate on the
 * DC-corrected x', ahead of the input-rate tune, the resampling stage, tfrec_amd_tune_streams and process_iq.  There is no reference
 * counterpart: this text is normative.  Exact integers:
 *   Windows.  Those of the DC blocker: L = 512 complex input samples, counted from the row's first submit or its last reset, never
 *     straddling a submit.  d[w] is the blocker's estimate for window w, (0, 0) on a context without the blocker (dc_windows = 0).
 *   Moments.  Per window, on the UNCLAMPED differences u = x - d[w] per rail: A[w] = sum u_I^2, B[w] = sum u_Q^2, C[w] = sum u_I u_Q.
 *     |u| <= 16383, so A, B <= 2^37 and |C| <= 2^37.  They follow exactly from five raw sums of one pass over the window (S_I, S_Q as
 *     for the blocker, M_II = sum x_I^2, M_QQ = sum x_Q^2, M_IQ = sum x_I x_Q):
 *         A = M_II - 2 d_I S_I + 512 d_I^2,  B = M_QQ - 2 d_Q S_Q + 512 d_Q^2,  C = M_IQ - d_I S_Q - d_Q S_I + 512 d_I d_Q.
 *   Sums.  K = iq_windows, 1 <= K <= 4096; lo = max(0, w - K + 1); SA, SB, SC = the sums of A, B, C over windows lo .. w, window w
 *     included (<= 2^49).
 *   Estimate.  In int64, with floor division and arithmetic shifts:
 *         s = max(0, bitlen(max(SA, SB)) - 31);  a = SA >> s, b = SB >> s, c = SC >> s;
 *         D = a b - c^2  (a, b < 2^31, |c| <= 2^31);  r = isqrt(D), the exact floor of the square root;
 *         t = floor((c 32768 + a) / (2 a));  g = floor((a 32768 + r) / (2 r)).
 *     t and g are Q14: C / A and A / sqrt(A B - C^2), rounded half up.  The window gets the IDENTITY t = 0, g = 16384 if a == 0,
 *     D <= 0, |t| > 4096, g < 12288 or g > 20480 (about +-14 degrees and +-25 %): a silent, a fully correlated or an absurd window is
 *     passed through unchanged.  These are conditions, not measurements.
 *   Apply.  On the clamped x' = clamp(x - d[w], -8192, 8191):  I'' = I';  v = (Q' 16384 - t I' + 8192) >> 14;
 *     Q'' = clamp((v g + 8192) >> 14, -8192, 8191) -- int32 throughout: |t I'| <= 2^25, |v| <= 10241, |v g| < 2^28.  Everything
 *     downstream is the text above applied to x''; its no-wrap arguments hold because |x''| <= 8192.
 *   State.  Per row the last K triples (A, B, C) and the window count, carried from submit to submit (beside the blocker's).  A
 *     stream restart does not touch it; tfrec_amd_reset_iq_rows clears it at the next submit; a row that a submit does not provide
 *     keeps it.  Results do not depend on how a row is cut into submits.
 *   Limits.  One frequency-flat correction per row, estimated on the assumption that the row's signals are proper (circular): a lone
 *     carrier at 0 Hz is not, so a recording with a DC offset wants dc_windows > 0; the first windows of a row are estimated from
 *     few samples.
 * tfrec_amd_create_iq: dc_windows within [0, 4096], 0 for no DC blocker; iq_windows within [1, 4096]; formats, rates, max_rows and
 * refusals (TFREC_AMD_F_INPUT_10X, an unknown format, a refused rate, a value out of range: TFREC_AMD_E_INVAL) as for
 * tfrec_amd_create_dc.  With dc_windows > 0, tfrec_amd_get_dc, tfrec_amd_read_dc and tfrec_amd_reset_dc_rows work as on a
 * tfrec_amd_create_dc context; with dc_windows = 0 they answer as on a context without a blocker.  The context is a format context
 * in every other respect, as a DC context is: tfrec_amd_read_stage0, levels, capture and events see the CORRECTED input; the
 * spectrum and the occupancy detector keep reading the caller's raw rows.  Memory (all in tfrec_amd_get_memory), beside the
 * blocker's where there is one: per FIFO set the table of (t, g), 4 bytes per window, and -- without the blocker -- the corrected
 * rows, max_rows * n_max * 4 bytes; per context a submit's five sums (32 bytes per window) and moments (24), the ring of moments
 * (max_rows * K * 24 bytes) and the counts.  Pinned by tfrec_amd/iqbal.py.  Contexts of every other constructor launch what they
 * launched before. */
int tfrec_amd_create_iq(const tfrec_amd_config *cfg, int32_t format, int32_t rate_p, int32_t rate_q, int32_t dc_windows, int32_t iq_windows,
			int32_t max_rows, tfrec_amd_ctx **out);
/* iq_windows and max_rows of a tfrec_amd_create_iq context; 0 and 0 on every other context. */
int tfrec_amd_get_iq(tfrec_amd_ctx *ctx, int32_t *iq_windows, int32_t *max_rows);
/* (t, g) of one input row of the OLDEST undrained submit, with the conventions of tfrec_amd_read_dc (waits for the submit; call it
 * BEFORE tfrec_amd_drain_events pops it; reading pops nothing): tg[2 * w] = t and tg[2 * w + 1] = g of the submit's window w, for
 * w < *n_windows = n_in / 512; cap_windows is the room in windows.  tg may be NULL with cap_windows 0 to fetch only *n_windows.
 * Errors: not a tfrec_amd_create_iq context, a row the submit did not use, n_windows NULL: TFREC_AMD_E_INVAL; the room too small
 * (or tg NULL): TFREC_AMD_E_INVAL, nothing is written, but *n_windows is set; nothing undrained or a poisoned context:
 * TFREC_AMD_E_STATE. */
int tfrec_amd_read_iq(tfrec_amd_ctx *ctx, int32_t row, int16_t *tg, size_t cap_windows, int *n_windows);
/* Clear the balancer's state of the listed rows (each within [0, max_rows); duplicates allowed; n == 0: nothing) at the NEXT
 * submit: their window count restarts at 0 there.  The DC blocker's state is tfrec_amd_reset_dc_rows's.  Submits already queued
 * are not affected; the streams that read the rows are not restarted.  Errors as tfrec_amd_reset_dc_rows: a NULL list with n > 0,
 * n < 0, a row out of range or a context without the balancer: TFREC_AMD_E_INVAL, and nothing is marked; a poisoned context:
 * TFREC_AMD_E_STATE. */
int tfrec_amd_reset_iq_rows(tfrec_amd_ctx *ctx, const int32_t *rows, int n);

/* Save and restore a stream's receiver state: everything one submit leaves for the next -- what
 * tfrec_amd_reset_streams restores, copied instead of filled -- as one self-describing blob per stream, so that a stream can
 * leave the context that holds it: into a recreated context after a poisoned one (from its last snapshot), into a context of
 * another n_streams, max_blocks or device, or into a later run.  A stream loaded into stream j of a context B continues there
 * exactly as it would have in its source: its events in B, behind those it produced before the save, are those of the
 * uninterrupted receiver in every field (seq, end_sample, the recorder's start_sample and the tunes' phases included).
 *
 * A blob is this 128-byte header (little endian, packed as declared) followed by an opaque payload of payload_bytes bytes;
 * tfrec_amd_stream_state_bytes is the whole blob's size in THIS context, a multiple of 16, the same for every stream.  The
 * header names nothing of the source context: no stream index, no device, no n_streams. */
#define TFREC_AMD_STATE_MAGIC 0x54534654u /* "TFST" */
#define TFREC_AMD_STATE_FORMAT 1u
typedef struct {            /* 128 bytes */
	uint32_t magic;             /*   0  TFREC_AMD_STATE_MAGIC */
	uint32_t format;            /*   4  TFREC_AMD_STATE_FORMAT */
	uint64_t version_hash;      /*   8  FNV-1a (64 bit) of the bytes of tfrec_amd_version(): a blob of another build is refused */
	/* the signature: what must be equal in the source and the target context */
	int32_t input_kind;         /*  16  0 u8 at 1.536 MS/s, 1 TFREC_AMD_F_INPUT_10X, 2 a resampling stage, 3 a format at 1/1, 4 decimated */
	int32_t format_in;          /*  20  TFREC_AMD_FMT_* of the input rows */
	int32_t format_pre;         /*  24  ... and of what the pre-stage reads (S16 behind an input correction) */
	int32_t rate_p, rate_q;     /*  28  the input rate 1536000 P / Q */
	int32_t tail_bytes;         /*  36  the front end's FIR history per stream */
	int32_t pre_bytes;          /*  40  the pre-stage's history per stream */
	uint32_t types_mask;        /*  44  the context's registered demodulators */
	uint32_t flags;             /*  48  the context's TFREC_AMD_F_SERIAL_CHAINS and TFREC_AMD_F_LEVELS, nothing else */
	uint32_t recorder;          /*  52  1: tfrec_amd_enable_capture was called */
	int32_t dc_windows;         /*  56  the DC blocker's K, 0 without one */
	int32_t iq_windows;         /*  60  the IQ balancer's K, 0 without one */
	uint32_t chain_state_bytes; /*  64  the size of one demodulator's carried record in this build */
	uint32_t payload_bytes;     /*  68  bytes behind the header */
	int64_t samples_since_restart;    /*  72  decimated samples the stream has run since its start or last restart */
	tfrec_amd_stream_config config;   /*  80  the stream's settings */
	int32_t tune_hz;            /*  96  tfrec_amd_tune_streams */
	int32_t tune_wide_hz;       /* 100  tfrec_amd_tune_streams_wide (0 in a context without the 10:1 stage) */
	int32_t tune_input_hz;      /* 104  tfrec_amd_tune_streams_input (0 in a context without an input-rate mixer) */
	uint8_t reserved[20];       /* 108  zero */
} tfrec_amd_state_header;
/* n_streams, max_blocks, max_events, the device, the pipeline layout and every flag but the two named are deliberately no part of
 * the signature: they may differ between the source and the target. */
int tfrec_amd_stream_state_bytes(tfrec_amd_ctx *ctx, size_t *bytes);
/* Save streams[0..n) (distinct) into blobs[i * bytes .. (i + 1) * bytes), bytes = tfrec_amd_stream_state_bytes.
 *   - Waits for everything queued, as tfrec_amd_sync does: the state saved is the state behind the LAST submit made.  That wait
 *     is the call's price; a context that never calls it runs exactly as before.
 *   - Drains nothing: undrained submits stay in the FIFO and drain unchanged, and the context continues as if it had not saved.
 *   - One kernel gathers the listed streams into a device staging buffer (made at the first save or load, n_streams blobs,
 *     counted by tfrec_amd_get_memory from then on), one copy brings it out.  Two saves without a submit between them give the
 *     same bytes.
 * Errors: a poisoned context, or a stream with a reset, configure, tune or map (or its row with a tfrec_amd_reset_dc_rows /
 * _iq_rows) pending since the last submit -- its state is about to be replaced: TFREC_AMD_E_STATE.  An index out of range or
 * listed twice, n < 0, a NULL pointer with n > 0, cap_bytes < n * bytes, a stream that reads another row than its own or whose row
 * another stream reads (tfrec_amd_map_streams; shared rows are not saved): TFREC_AMD_E_INVAL.  Nothing is written then. */
int tfrec_amd_save_streams(tfrec_amd_ctx *ctx, const int32_t *streams, int n, void *blobs, size_t cap_bytes);
/* Load blobs[i] (n blobs of tfrec_amd_stream_state_bytes each, bytes >= n * that) into streams[i] (distinct) of this context.
 *   - Every blob is validated before anything is touched: magic, format, version hash, the signature against this context's,
 *     payload_bytes, samples_since_restart >= 0, the settings and the tunes under the checks of tfrec_amd_configure_streams and
 *     the tune calls.  Any refusal leaves the context exactly as it was.
 *   - Then it waits as a save does and scatters the payloads with the kernel of the save (one table of the inventory serves both
 *     directions).  The settings and tunes are applied as tfrec_amd_configure_streams and the tune calls would apply them, but
 *     without their restart; the stream's sample origin becomes (samples submitted so far) - samples_since_restart, so that
 *     end_sample, seq, the recorder's start_sample and the phase of every mixer continue.  Submits still in the FIFO drain with
 *     the origins they ran with.
 *   - Not carried: context-wide counters (tfrec_amd_get_stats, _get_fm_stats, timings) and side-output records of submits
 *     already made.
 * Errors: a poisoned context, or a listed stream with a restart pending (it would replace what was loaded): TFREC_AMD_E_STATE;
 * an index out of range or listed twice, a mapped stream as for a save, n < 0, a NULL pointer with n > 0, bytes too small, or a
 * blob refused by the validation: TFREC_AMD_E_INVAL (tfrec_amd_last_error says which field). */
int tfrec_amd_load_streams(tfrec_amd_ctx *ctx, const int32_t *streams, int n, const void *blobs, size_t bytes);

/* Wait for submitted work. */
int tfrec_amd_sync(tfrec_amd_ctx *ctx);

/* Replaces the calls `dec->flush(rssi, offset)` inside tfa1_demod::demod (tfa1.cpp:180), tfa2_demod::demod
 * (tfa2.cpp:434) and whb_demod::demod (whb.cpp:696): one tfrec_amd_event per call site and window.
 * Wait for the OLDEST submit that has not been drained yet, then copy its events to out[0..cap), ordered by
 * (stream, slot, seq).  *n_out = number written (0 if nothing was submitted).  Returns TFREC_AMD_E_OVERFLOW if the
 * device buffer or cap was too small (the events that fit are still returned; the others are lost -- the decoder state and
 * the flush ordinals `seq` move on, so a gap in seq shows where).
 * Submits and drains form a FIFO of depth TFREC_AMD_FIFO_DEPTH (4): a caller may queue submits k+1 .. k+3 before
 * draining submit k, so that the GPU works on them (front end of k+2, filter stage of k+1 and slicer/decoder stage of
 * k run beside each other, and the front end of k+3 is already queued when that of k+2 ends: with three, the front-end
 * stream idled from then until the host had drained k and submitted again) while the host copies and dispatches k's
 * events; one more undrained submit is refused with TFREC_AMD_E_STATE.  Every queued submit owns a full set of
 * intermediate buffers (~7 GB at 1024 streams x 48 blocks).  Alternating submit / drain behaves as one would expect. */
int tfrec_amd_drain_events(tfrec_amd_ctx *ctx, tfrec_amd_event *out, int cap, int *n_out);

/* Number of events of the oldest undrained submit (waits for it). */
int tfrec_amd_pending_events(tfrec_amd_ctx *ctx, int *n);

/* Level meter (TFREC_AMD_F_LEVELS): what a receiver saw, whether or not it decoded anything -- per stream s and per
 * block b (TFREC_AMD_BLOCK_DEC decimated samples) of a submit one record of exact integers.  I, Q are the decimated int16 samples
 * tfrec_amd_read_decimated returns; pwr = |I| + |Q| is fsk_demod::process's trigger quantity (fm_demod.cpp:45). */
typedef struct {            /* 32 bytes */
	uint64_t energy;        /* sum over the block's 8192 decimated samples of I*I + Q*Q  (<= 2^44) */
	uint32_t pwr_sum;       /* sum of pwr (<= 2^29) */
	int32_t  pwr_max;       /* largest pwr in the block */
	int32_t  n_over;        /* samples with pwr > thresh (tfa1.cpp:147, tfa2.cpp:351, whb.cpp:636), thresh = the field below */
	int32_t  triggered;     /* fm_demod.cpp:52: samples at which at least one registered demodulator of this stream returned non-zero */
	int32_t  thresh;        /* the trigger threshold in force DURING this block */
	int32_t  triggered_avg; /* fm_demod.cpp:58, after this block */
} tfrec_amd_level;
/*   triggered: a demodulator returns non-zero while its timeout counter runs -- set to its window W at every sample with
 *     pwr > thresh, counted, then decremented (tfa1.cpp:147-164, tfa2.cpp:351-375, whb.cpp:636-657).  All demodulators of a stream
 *     share the trigger test, so sample n counts iff some sample n' of this stream has n - W < n' <= n, pwr[n'] > the thresh in
 *     force at n', and n' at or after the stream's start or last restart; W is the LARGEST window of the stream's own registered
 *     demodulators: 400 for TFA_1, (int)(16 * 384000 / baud) for TFA_2 (356), TFA_3 (640) and TX22 (694), 512 for WHB.  A trigger
 *     carries over block and submit boundaries.  The same quantity drives the auto threshold.
 *   triggered_avg, thresh: the recurrence of fm_demod.cpp:58-73 from triggered_avg = 0, runs = 0 and thresh = the stream's setting
 *     (500 in auto mode): per block runs++, triggered_avg = (31 * triggered_avg + triggered) / 32 -- in BOTH modes, as the reference
 *     computes it unconditionally --, and in auto mode only, when runs % 4 == 0: triggered_avg >= 512 raises thresh by 2, else
 *     triggered_avg <= 256 with thresh > 50 lowers it by 2.  On an auto stream the last record's thresh, stepped once more, is
 *     what tfrec_amd_read_thresh returns.
 *   A restart (reset, configure, tune, map, wide tune, input tune) returns the stream's level state to those starting values at
 *     the cut, and no trigger is carried over it.  Results do not depend on how a stream is cut into submits.
 *   Valid on every kind of context and in every mode (both layouts, _SERIAL_CHAINS, _BITS, _ALL_FLUSHES, _TIMING, _INPUT_10X, rate
 *     and format contexts): the records are defined on the decimated samples and the final trigger mask alone.  The two kernels that
 *     compute them run behind the front end on a low-priority stream of their own; the events do not depend on them.
 *   Memory: n_streams * max_blocks * 32 bytes of device memory per FIFO slot (TFREC_AMD_FIFO_DEPTH of them) and 16 bytes per stream
 *     of carried state; no page-locked host copy (the call below copies into `out`).  Pinned by tfrec_amd/levels.py.
 * tfrec_amd_read_levels: the levels of the OLDEST undrained submit (waits for it, like tfrec_amd_pending_events; call it BEFORE
 * tfrec_amd_drain_events pops that submit): out[s * n_blocks + b], n_streams * n_blocks records (cap: the room in `out`, in
 * records); *n_blocks_out = that submit's n_blocks.
 * Errors: a context without TFREC_AMD_F_LEVELS: TFREC_AMD_E_INVAL; nothing undrained: TFREC_AMD_E_STATE; cap too small or a NULL
 * pointer: TFREC_AMD_E_INVAL, and nothing is written; a poisoned context: TFREC_AMD_E_STATE. */
int tfrec_amd_read_levels(tfrec_amd_ctx *ctx, tfrec_amd_level *out, size_t cap, int *n_blocks_out);

/* Squelched recorder (tfrec_amd_enable_capture): the IQ of every trigger window -- exactly the decimated samples the
 * demodulators were run on, packed, with their positions.  Exact integers only; no new arithmetic.
 *   Captured samples: for stream s, decimated sample n is counted since the stream's start or last restart, as end_sample is.
 *     Sample n is captured iff it is `triggered` in the sense of tfrec_amd_level: some n' with n - W < n' <= n, at or after the
 *     last restart, has pwr[n'] > the thresh in force at n'.  W is the largest window of the stream's own registered demodulators
 *     (400 / 356 / 640 / 694 / 512).  These are the samples for which at least one demodulator::demod call of that stream ran with
 *     its timeout counter live.  There is no pre-roll: the demodulators see none either -- a run begins AT the sample that
 *     triggered, not before it.
 *   Runs: a run is a maximal set of consecutive captured samples of one stream within one submit.  A trigger that carries over a
 *     submit boundary gives two runs: the second starts at the submit's first sample and has TFREC_AMD_RUN_CONTINUES set (the sample
 *     just before the submit was captured too, and no restart lies between).  A run that reaches the submit's last sample has
 *     TFREC_AMD_RUN_OPEN set.
 *   Outputs per submit: a run table ordered by (stream, start_sample), and a sample pool: the runs' int16 (I, Q) pairs, packed back
 *     to back in table order, the values exactly those tfrec_amd_read_decimated returns.  pool_offset is therefore the exclusive
 *     prefix sum of n_samples in table order: the layout is deterministic (no atomic decides an order).
 *   Cutting: the set of (stream, n, I, Q) over all runs does not depend on how a stream is cut into submits; only the split of
 *     runs at submit boundaries and the two flags do.
 *   Restarts: any restart (reset, configure, tune, map, wide tune, input tune) drops the carried trigger at the cut, as for the
 *     levels: no CONTINUES run follows a restart, and start_sample counts from 0 again.
 *   Validity: every kind of context and every mode, as the level meter: it is defined on the decimated samples and the final
 *     trigger mask alone.  Its three kernels run behind the front end on a low-priority stream of their own; events and levels do
 *     not depend on them.  Pinned by tfrec_amd/capture.py. */
#define TFREC_AMD_RUN_CONTINUES 1u
#define TFREC_AMD_RUN_OPEN 2u
typedef struct {            /* 32 bytes */
	uint32_t stream;
	uint32_t flags;         /* TFREC_AMD_RUN_CONTINUES 1, TFREC_AMD_RUN_OPEN 2 */
	int64_t  start_sample;  /* first captured sample, counted like end_sample */
	uint32_t n_samples;
	int32_t  thresh;        /* the threshold in force at start_sample */
	uint64_t pool_offset;   /* index of the run's first (I, Q) pair in the sample pool */
} tfrec_amd_run;
/* Turn the recorder on: allowed only before the first submit (after it: TFREC_AMD_E_STATE).  Allocates, per FIFO set
 * (TFREC_AMD_FIFO_DEPTH of them), max_runs * 32 bytes for the table, max_samples * 4 bytes for the pool and a 16-byte header, and
 * once per context 16 bytes of carried state, 24 bytes of counts and bases and (max_blocks * 8192 / 356 + 3) * 20 bytes of
 * staging per stream (a stream cannot have more runs in a submit: all but its first and last are at least 356 samples long);
 * tfrec_amd_get_memory counts all of it.  tfrec_amd_config has no spare field, so this is a call and not a flag.
 * Errors: a NULL context, a zero argument or a second call: TFREC_AMD_E_INVAL; TFREC_AMD_E_NOMEM as elsewhere (the context stays
 * usable, without the recorder); a poisoned context: TFREC_AMD_E_STATE.  A call that fails leaves the context exactly as it was
 * before it: it holds nothing for the recorder, tfrec_amd_get_memory reports what it reported, and a later call is a first one.
 * A context on which it was never called creates no stream, event or buffer for this and launches what it launched before. */
int tfrec_amd_enable_capture(tfrec_amd_ctx *ctx, uint32_t max_runs, uint64_t max_samples);
/* The captures of the OLDEST undrained submit (waits for it; like tfrec_amd_read_levels, call it BEFORE tfrec_amd_drain_events pops
 * that submit; reading pops nothing).  runs[0 .. *n_runs), samples[2 * pool_offset ..] = I, Q of a run's pairs; cap_runs and
 * cap_pairs are the room in runs (entries) and samples (pairs).  samples may be NULL with cap_pairs 0 to fetch only the table and
 * the counts.
 * Errors: capture not enabled, or a NULL ctx, runs (with cap_runs > 0), n_runs or n_pairs: TFREC_AMD_E_INVAL; nothing undrained or
 * a poisoned context: TFREC_AMD_E_STATE; the caller's room too small: TFREC_AMD_E_INVAL, nothing written, but *n_runs / *n_pairs
 * set, so that the caller can size and call again.
 * Device-side overflow -- the submit has more runs than max_runs or more pairs than max_samples --: TFREC_AMD_E_OVERFLOW, *n_runs /
 * *n_pairs are the TRUE totals, and the call delivers the longest prefix of the table that fits both limits, whole runs only
 * (the room needed is that prefix's; where cap_runs exceeds it, the entry behind the prefix is zeroed: n_samples == 0 ends the
 * table, as no run is empty).  Events, levels and carried state are unaffected: the next submit captures normally, and its
 * CONTINUES flag is still correct. */
int tfrec_amd_read_captures(tfrec_amd_ctx *ctx, tfrec_amd_run *runs, size_t cap_runs, uint32_t *n_runs, int16_t *samples,
			    size_t cap_pairs, uint64_t *n_pairs);

/* Channel-rate input: a context whose input rows already hold what process_iq produces -- little-endian int16 (I, Q)
 * pairs at 384 kS/s, from tfrec_amd_read_captures, tfrec_gpu -S or an upstream channeliser.  A block is 8192 pairs = 32768 bytes:
 * tfrec_amd_input_bytes returns n_blocks * 32768, tfrec_amd_get_input_rate 1/4, tfrec_amd_get_input_format TFREC_AMD_FMT_DEC16
 * (which tfrec_amd_create_format keeps refusing).  The stride and alignment rules of the submits are unchanged.
 *   Definition.  Per component v' = max(v, -32767), so that I*I + Q*Q and every product downstream stays inside int32; dec[n] =
 *     (I', Q') is what tfrec_amd_read_decimated returns and what enters fsk_demod::process; mask bit n = |I'| + |Q'| > thresh of the
 *     stream (the context's or its tfrec_amd_stream_config's; an auto stream's mask is rewritten block by block as on every
 *     context).  The sample ahead of a submit's first one is the stream's last pair of the submit before, (0, 0) at the start and
 *     after any restart: 4 bytes of carried state per stream.
 *   No filter stage: no FIR, no history, no pre-stage.  filter_type is accepted, in the config and per stream, and has no effect.
 *   Parity is pinned for inputs the decimator can produce (what tfrec_amd_read_decimated returns of any other context: fed back,
 *     they give that context's events bit for bit).  For other int16 input the definition is the reference's arithmetic on those
 *     values.
 *   Works: reset, configure, tfrec_amd_map_streams (the kernel looks the row up), levels, the recorder, both layouts,
 *     _SERIAL_CHAINS, _BITS, _ALL_FLUSHES, _TIMING.  Refused with TFREC_AMD_E_INVAL: TFREC_AMD_F_INPUT_10X; the three tunes (they are
 *     defined ahead of process_iq); tfrec_amd_enable_spectrum (its bounds assume |x| <= 8192); tfrec_amd_read_stage0.
 * Contexts of the older constructors launch what they launched before, with the arguments they had. */
#define TFREC_AMD_FMT_DEC16 16
int tfrec_amd_create_decimated(const tfrec_amd_config *cfg, tfrec_amd_ctx **out);
/* The recorder's missing sample: with it a capture holds everything its stream's flush events depend on.  Call after
 * tfrec_amd_enable_capture and before the first submit; max_runs * 4 bytes of device memory per FIFO set, counted in
 * tfrec_amd_get_memory.  Errors: no recorder or a second call: TFREC_AMD_E_INVAL; after the first submit or a poisoned context:
 * TFREC_AMD_E_STATE; TFREC_AMD_E_NOMEM as elsewhere; a call that fails leaves the context exactly as it was.  A recorder on which
 * it was never called holds and launches what it did. */
int tfrec_amd_enable_capture_pre(tfrec_amd_ctx *ctx);
/* pre[2 i], pre[2 i + 1] = the decimated (I, Q) just ahead of runs[i].start_sample of the table tfrec_amd_read_captures returns for
 * the same submit: the sample before it inside the submit, for a run at the submit's first sample the stream's last sample of the
 * submit before, and (0, 0) where nothing precedes -- a stream's start or restart.  Conventions of tfrec_amd_read_captures: the
 * OLDEST undrained submit, read BEFORE the drain that pops it; cap_runs is the room in pairs; *n_runs the submit's true run count; on
 * a device-side overflow TFREC_AMD_E_OVERFLOW and the same delivered prefix.  Errors: not enabled, NULL ctx / n_runs / pre (with
 * cap_runs > 0), room too small (nothing written, *n_runs set): TFREC_AMD_E_INVAL; nothing undrained or poisoned: TFREC_AMD_E_STATE. */
int tfrec_amd_read_capture_pre(tfrec_amd_ctx *ctx, int16_t *pre, size_t cap_runs, uint32_t *n_runs);
/* Sparse submits on a channel-rate context: allowed only before the first submit.  Per FIFO set, on the device and page-locked on
 * the host alike: max_runs * 20 bytes (table and pre), max_samples * 4 bytes (pool), (n_streams + 1) * 4 and n_streams * 8 bytes;
 * tfrec_amd_get_memory counts all of it.  Errors: not a tfrec_amd_create_decimated context, a zero argument, max_runs >= 2^31 or a
 * second call: TFREC_AMD_E_INVAL; after the first submit: TFREC_AMD_E_STATE; TFREC_AMD_E_NOMEM as elsewhere; a failed call leaves
 * the context as it was. */
int tfrec_amd_enable_runs_input(tfrec_amd_ctx *ctx, uint32_t max_runs, uint64_t max_samples);
/* Exactly tfrec_amd_submit_host of the expanded rows, with M = n_blocks * 8192: every sample (0, 0); run i's pairs
 * (samples[2 * pool_offset ..]) at [start_sample, start_sample + n_samples) of row runs[i].stream; pre[2 i], pre[2 i + 1] at
 * start_sample - 1 when start_sample > 0; when start_sample == 0, pre[i] is that stream's "sample ahead of the submit" for this
 * submit instead of the carried pair (a stream that restarts at this submit still gets (0, 0)).  Only the table, the pool and pre
 * cross to the device (host memory, copied before the call returns).  FIFO, poisoning and the n_blocks rules are those of the other
 * submits.  Rules, checked before anything is queued (a violation: TFREC_AMD_E_INVAL, nothing queued, no state changed):
 * start_sample is submit-relative, within [0, M); n_samples >= 1 and start_sample + n_samples <= M; stream < n_streams; the table is
 * ordered by (stream, start_sample); at least one sample lies between two runs of a row; pool_offset is the exclusive prefix sum of
 * n_samples and n_pairs their total; n_runs <= max_runs and n_pairs <= max_samples; a mapped context is refused (the dense submit
 * serves those).  flags and thresh of the entries are ignored.  tfrec_amd/decin.py (expand, check, rebase) restates all of it. */
int tfrec_amd_submit_runs(tfrec_amd_ctx *ctx, const tfrec_amd_run *runs, uint32_t n_runs, const int16_t *samples, uint64_t n_pairs,
			  const int16_t *pre, int n_blocks);

/* Burst meter (tfrec_amd_enable_burst_meter): for every run of the recorder's table -- every trigger window, decoded or
 * not, of any protocol or none -- where its carrier sits relative to the receive frequency and how wide its FSK is: an exact integer
 * histogram of the instantaneous frequency.  It sits on the recorder as tfrec_amd_enable_capture_pre does.  There is no reference
 * counterpart: this text is normative, tfrec_amd/burst.py restates it.  Exact integers only.
 *   Samples:  for entry e of a submit's table (tfrec_amd_run: stream s, submit-relative start a, n = n_samples, flags), z[k] = (I, Q) is
 *             the decimated pair at submit-relative index a + k, 0 <= k < n -- exactly the values tfrec_amd_read_decimated returns.
 *             z[-1] is the pair at a - 1; for a == 0 the stream's last pair of the submit before.
 *   Products: over k = k0 .. n-1, k0 = 0 if flags & TFREC_AMD_RUN_CONTINUES, else 1: the product of a trigger's first sample with the
 *             noise sample ahead of it is left out, and the product across a submit boundary is counted once, in the CONTINUES piece.
 *             dot = I[k] I[k-1] + Q[k] Q[k-1],  crs = Q[k] I[k-1] - I[k] Q[k-1]  in int64 (|dot|, |crs| <= 2^31): fm_dev's cr and cj
 *             (dsp_stuff.cpp:284-289).  A tone above the receive frequency gives crs > 0.
 *   Bin:      a product with dot == 0 && crs == 0 is skipped.  Otherwise, with C[k] = round(32767 cos(2 pi k / 4096)), S[k] = C[(k - 1024)
 *             mod 4096] (tfrec_amd_tune_streams' table, no other), its bin is the j in 0..63 that maximises dot C[64 j] + crs S[64 j]
 *             (int64, < 2^47), the lowest j on a tie.  Bin j is the direction 2 pi j / 64: 6000 b Hz at 384 kS/s, b = j for j < 32,
 *             else j - 64.  Any evaluation that provably returns the same j is allowed.
 *   Record:   the fields below; pwr_max and energy run over all n samples, n_products, sum_dot, sum_crs and hist over the counted
 *             products.  The record repeats the table entry's fields, so a caller needs neither the table nor the pool.
 *   Cutting:  a burst is a chain of pieces: piece i + 1 has CONTINUES, piece i OPEN, on the same stream.  Merging a chain adds
 *             n_samples, n_products, the sums, energy and hist and takes the largest pwr_max; the result does not depend on how
 *             the stream was cut into submits.  A restart drops the chain, as it drops the carried trigger.  A chain whose last piece
 *             is OPEN and which the next submit does not continue (no CONTINUES piece of its stream) ended with that submit's last
 *             sample: the merged record is complete and its OPEN is cleared, as the uncut run's is.  This holds for every record
 *             that is merged by chains (tfrec_amd_envelope, tfrec_amd_clock, tfrec_amd_track).
 *   Summary (what a caller makes of a record; normative for tfrec_gpu -M and burst.py):  P = n_products, thr = (P + 15) / 16; bin j is
 *             occupied iff P > 0 and hist[j] >= thr.  None occupied: no carrier (noise spreads over the bins).  Otherwise lo, hi = the
 *             smallest and largest signed index b of an occupied bin, centre_hz = 3000 (lo + hi), deviation_hz = 3000 (hi - lo).
 *             Signals near +-192 kHz wrap around; they lie far outside the channel filter.  The factor 16 was chosen on the
 *             synthetic golden scenes; neither it nor the usefulness of centre and deviation has been measured on real recordings.
 *   Sign:     the reference's TFA_2 line prints "Offset" = -1536.0 * offset / 131072 kHz (tfa2.cpp:169) with offset the decoder's mean
 *             of fm_dev: it is positive for a carrier BELOW the receive frequency, so it has the opposite sign of centre_hz.  Golden
 *             TFA_2 scene, first telegram: received 20 kHz higher (tfrec_amd_tune_streams +20000, the carrier 20 kHz below) the
 *             reference prints Offset +26.2 kHz and centre_hz is -21000; received 20 kHz lower, -13.7 kHz and +21000; untuned, +6.2
 *             kHz and +3000. */
typedef struct {            /* 320 bytes */
	uint32_t stream;        /* these five: copied from the table entry */
	uint32_t flags;
	int64_t  start_sample;
	uint32_t n_samples;
	int32_t  thresh;
	int32_t  pwr_max;       /* max over all n samples of |I| + |Q| */
	uint32_t n_products;    /* products counted = the sum of hist */
	int64_t  sum_dot;       /* over the counted products; |sum| <= 2^56 */
	int64_t  sum_crs;
	uint64_t energy;        /* sum over all n samples of I*I + Q*Q */
	uint32_t hist[64];      /* the bin counts */
	uint32_t reserved[2];   /* 0 */
} tfrec_amd_burst;
/* Turn the meter on: after tfrec_amd_enable_capture, before the first submit.  max_runs * 320 bytes of device memory per FIFO set,
 * counted in tfrec_amd_get_memory.  Errors: no recorder or a second call: TFREC_AMD_E_INVAL; after the first submit or a poisoned
 * context: TFREC_AMD_E_STATE; TFREC_AMD_E_NOMEM as elsewhere; a call that fails leaves the context exactly as it was.  A context on
 * which it was never called holds and launches what it did.  Valid on every kind of context and in every mode, as the recorder is; on
 * a tfrec_amd_submit_runs submit the samples between the runs are (0, 0), and their products fall to the zero rule.  Its two kernels
 * run on the recorder's low-priority stream behind its own. */
int tfrec_amd_enable_burst_meter(tfrec_amd_ctx *ctx);
/* out[i] = the record of entry i of the table tfrec_amd_read_captures returns for the same submit.  Conventions of
 * tfrec_amd_read_capture_pre: the OLDEST undrained submit, read BEFORE the drain that pops it; reading pops nothing; cap_runs is the
 * room in records; *n_runs the submit's true run count; out may be NULL with cap_runs 0 to fetch the count alone.  The meter reads the
 * decimated samples, not the pool: records are delivered for every entry below min(n_runs, max_runs), whatever max_samples is (a
 * recorder with a pool of one pair runs the meter alone).  n_runs > max_runs: TFREC_AMD_E_OVERFLOW with that prefix delivered.
 * Errors: not enabled, NULL ctx / n_runs / out (with cap_runs > 0), room too small (nothing written, *n_runs set): TFREC_AMD_E_INVAL;
 * nothing undrained or poisoned: TFREC_AMD_E_STATE. */
int tfrec_amd_read_bursts(tfrec_amd_ctx *ctx, tfrec_amd_burst *out, size_t cap_runs, uint32_t *n_runs);

/* Burst envelope (tfrec_amd_enable_burst_envelope): for every run of the recorder's table how long the burst itself was
 * -- a run's n_samples includes the trigger's hold of W - 1 samples of noise behind the burst --, how far it stood above that noise,
 * and whether it was one clean burst or a broken one.  It sits on the recorder as the burst meter does and is independent of it.
 * There is no reference counterpart: this text is normative, tfrec_amd/envelope.py restates it.  Exact integers only.
 *   Samples:  for entry e of a submit's table (tfrec_amd_run: stream s, submit-relative start a, n = n_samples, flags), z[k] = (I, Q) is
 *             the decimated pair at submit-relative index a + k, 0 <= k < n, as tfrec_amd_read_decimated returns it.
 *   Over:     over[k] is bit a + k of the stream's FINAL trigger mask of that submit: |I| + |Q| > the threshold in force at that sample,
 *             the quantity tfrec_amd_level.n_over counts.  The mask of an auto stream is the one the threshold pass rewrote block by
 *             block.  On a tfrec_amd_submit_runs submit the samples between the runs are (0, 0) and never over.
 *   Record:   n_over = the number of k with over[k];  last_over = the largest such k, or -1 if there is none (a run without CONTINUES
 *             starts at an over sample, so -1 occurs only in CONTINUES pieces).  head = the samples k <= last_over, tail = the samples
 *             k > last_over: a run's last W - 1 samples are tail by construction, the burst's own noise reference.
 *             energy_head, energy_tail = the sums of I*I + Q*Q over head and over tail.
 *             A gap is a maximal stretch of not-over samples inside the head with an over sample on both sides within this piece:
 *             n_gaps counts them, max_gap is the longest (0 if none).  lead_not_over = the not-over samples before the piece's first
 *             over sample (n if there is none): 0 unless the piece CONTINUES; it is what rebuilds a gap that straddles a cut.
 *             dot_*, crs_*, nprod_*: the burst meter's products (tfrec_amd_burst: Products, with its k0, its zero rule and its z[-1]),
 *             product k counted in head if k <= last_over, else in tail: the mean frequency of the burst without its noise tail.
 *   Cutting:  a burst is a chain of pieces: piece i + 1 has CONTINUES, piece i OPEN, on the same stream.  Two adjacent pieces A, B (or
 *             a merged chain A and the next piece B) merge into the record the uncut run would have had:  n = nA + nB;  n_over adds;
 *             if B has an over sample (last_over_B >= 0): last_over = nA + last_over_B, head = head_A + tail_A + head_B, tail = tail_B;
 *             else last_over = last_over_A, head = head_A, tail = tail_A + tail_B -- for the energies, the product sums and counts.
 *             lead_not_over = lead_A if A has an over sample, else nA + lead_B.  With j = (nA - 1 - last_over_A) + lead_B, the stretch
 *             joined at the cut:  n_gaps = gaps_A + gaps_B + (A and B both have an over sample and j > 0), max_gap = max(max_A, max_B,
 *             j if both have one).  A stretch counts once; one that ends up behind the chain's final last_over is tail, not a gap.
 *             stream, start_sample, thresh and CONTINUES are A's, OPEN is B's.  The result does not depend on how the stream was cut
 *             into submits.  A restart drops the chain, as it drops the carried trigger.
 *   Summary (what a caller makes of a merged record; normative for tfrec_gpu -Q and envelope.py):  len = last_over + 1, the burst's
 *             length;  n_tail = n - len;  ratio_c = floor(100 * energy_head * n_tail / (energy_tail * len)) in 128-bit integers: the
 *             mean power of the burst over the mean power of its noise tail, in hundredths.  It is defined only if the chain is not
 *             OPEN, len > 0, energy_tail > 0 and n_tail >= 64 (a condition, not a measurement: a shorter tail -- a chain cut off by
 *             the input's end or by a restart -- is no noise reference).  snr_db = 10 log10(ratio_c / 100) in host double, printed
 *             with one decimal; undefined when ratio_c is undefined or 0.  snr_db is presentation only: its last digit may depend on
 *             the host's libm at a rounding tie; every exact comparison is made on ratio_c. */
typedef struct {            /* 128 bytes */
	uint32_t stream;        /* these five: copied from the table entry */
	uint32_t flags;
	int64_t  start_sample;
	uint32_t n_samples;
	int32_t  thresh;
	uint32_t n_over;        /* samples with over[k] */
	int32_t  last_over;     /* the largest k with over[k]; -1: none */
	uint64_t energy_head;   /* sum of I*I + Q*Q over k <= last_over */
	uint64_t energy_tail;   /* ... over k > last_over */
	uint32_t n_gaps;
	uint32_t max_gap;
	uint32_t lead_not_over;
	uint32_t nprod_head;    /* products counted with k <= last_over */
	int64_t  dot_head;
	int64_t  crs_head;
	int64_t  dot_tail;
	int64_t  crs_tail;
	uint32_t nprod_tail;
	uint32_t reserved[7];   /* 0 */
} tfrec_amd_envelope;
/* Turn the envelope on: after tfrec_amd_enable_capture, before the first submit.  max_runs * 128 bytes of device memory per FIFO set,
 * counted in tfrec_amd_get_memory.  Errors: no recorder or a second call: TFREC_AMD_E_INVAL; after the first submit or a poisoned
 * context: TFREC_AMD_E_STATE; TFREC_AMD_E_NOMEM as elsewhere; a call that fails leaves the context exactly as it was.  A context on
 * which it was never called holds and launches what it did.  Independent of tfrec_amd_enable_burst_meter: either, both or neither.
 * Valid on every kind of context and in every mode, as the recorder is.  Its three kernels run on the recorder's low-priority stream
 * behind its own and behind the burst meter's. */
int tfrec_amd_enable_burst_envelope(tfrec_amd_ctx *ctx);
/* out[i] = the record of entry i of the table tfrec_amd_read_captures returns for the same submit.  Conventions of tfrec_amd_read_bursts:
 * the OLDEST undrained submit, read BEFORE the drain that pops it; reading pops nothing; cap_runs is the room in records; *n_runs the
 * submit's true run count; out may be NULL with cap_runs 0 to fetch the count alone.  It reads the decimated samples and the mask, not
 * the pool: records are delivered for every entry below min(n_runs, max_runs), whatever max_samples is.  n_runs > max_runs:
 * TFREC_AMD_E_OVERFLOW with that prefix delivered.  Errors: not enabled, NULL ctx / n_runs / out (with cap_runs > 0), room too small
 * (nothing written, *n_runs set): TFREC_AMD_E_INVAL; nothing undrained or poisoned: TFREC_AMD_E_STATE. */
int tfrec_amd_read_burst_envelopes(tfrec_amd_ctx *ctx, tfrec_amd_envelope *out, size_t cap_runs, uint32_t *n_runs);

/* Burst clock (tfrec_amd_enable_burst_clock): for every run of the recorder's table how fast the burst is keyed -- the
 * one property that separates the five protocols (38400, 17240, 9600, 8842 and 6000 bit/s) from each other and from foreign
 * transmitters.  It sits on the recorder as the burst meter and the envelope do and is independent of both.  There is no reference
 * counterpart: this text is normative, tfrec_amd/clock.py restates it.  Exact integers only.
 *   Samples:  for entry e of a submit's table (tfrec_amd_run: stream s, submit-relative start a, n = n_samples, flags), z[m] = (I, Q) is
 *             the decimated pair at submit-relative index m, as tfrec_amd_read_decimated returns it.
 *   Segments: segment q is the samples [1024 q, 1024 q + 1024); it counts for the entry iff it lies wholly inside [a, a + n).  Every
 *             submit is a whole number of 8192-sample blocks and start_sample counts from a restart at a submit boundary, so a
 *             submit-relative multiple of 1024 is one in start_sample terms: a segment never straddles a cut, and it is whole in a
 *             piece iff it is whole in the uncut run.  Nothing outside the segment is read: no prevdec, no pair ahead of the run.
 *   Products: with m' = m mod 1024: for m' >= 1, dot[m] = I[m] I[m-1] + Q[m] Q[m-1] and crs[m] = Q[m] I[m-1] - I[m] Q[m-1] (the burst
 *             meter's products), in 64 bits; |dot|, |crs| <= 2^31.  mx = the largest |dot| or |crs| of the segment.  mx == 0: the
 *             segment is SILENT, counts in n_silent and adds nothing else.  Otherwise sh = max(0, bitlength(mx) - 15) (bitlength(2^31)
 *             = 32), d = dot >> sh, c = crs >> sh, arithmetic shifts: -2^15 <= d, c < 2^15.
 *   Signal:   for m' >= 2, g[m] = d[m] d[m-1] + c[m] c[m-1], |g| <= 2^31, and g16[m] = min(g[m] >> 16, 32767), an int16 (the minimum
 *             binds only where all four factors are -2^15);  g16[m] = 0 for m' < 2.  This is the real part of the second-order
 *             product: it dips at every frequency transition, does not depend on the carrier offset, and is weighted by the fourth
 *             power of the amplitude, so a run's noise tail does not count; the shift normalises each segment by its own peak.
 *   Spectrum: for bins j = 4 .. 131 (375 j Hz; array index j - 4):  X_re = sum over the segment of g16[m] C[(4 j m') mod 4096], X_im
 *             likewise with S -- C, S the tune table of tfrec_amd_tune_streams --, |X| < 2^40;  P_j = (X_re >> 16)^2 + (X_im >> 16)^2
 *             < 2^49.
 *   Record:   n_segments = the entry's counted segments that are not silent, n_silent = those that are, spec[j - 4] = the sum of P_j
 *             over the former.
 *   Cutting:  a burst is a chain of pieces as for tfrec_amd_burst.  Merging adds n_samples, n_segments, n_silent and spec (spec
 *             saturates at 2^64 - 1, which cannot happen below 2^15 segments); stream, start_sample, thresh and CONTINUES are the
 *             first piece's, OPEN is the last one's.  By the segment rule the result is the uncut run's record.  A restart drops the
 *             chain.
 *   Summary (what a caller makes of a merged record; normative for tfrec_gpu -C and clock.py), in 128-bit integers, P[j] = spec[j - 4]:
 *             the band is j = 12 .. 128 (4500 .. 48000 Hz, 117 bins), tot its sum; the summary is undefined iff n_segments == 0 or tot
 *             == 0.  jp = the lowest j of the band's maximum;  num = P[jp+1] - P[jp-1], den = 2 P[jp] - P[jp-1] - P[jp+1];  off =
 *             floor((375 num + den) / (2 den)) if den > 0 and neither neighbour exceeds P[jp], else 0 (floor for a negative numerator
 *             too);  clock_hz = 375 jp + off;  quality_c = floor(100 * 117 * P[jp] / tot), the peak over the band's mean in
 *             hundredths.  The resolution is the 375 Hz bin, off a refinement; a rate above 48 kHz or below 4.5 kHz is not found; on a
 *             preamble or Manchester-like data a harmonic or the half rate may win; no quality threshold is built in.  Neither the
 *             band, the segment length nor the usefulness of quality_c has been measured on real recordings. */
typedef struct {            /* 1056 bytes */
	uint32_t stream;        /* these five: copied from the table entry */
	uint32_t flags;
	int64_t  start_sample;
	uint32_t n_samples;
	int32_t  thresh;
	uint32_t n_segments;    /* counted segments that are not silent */
	uint32_t n_silent;      /* counted segments whose every product is zero */
	uint64_t spec[128];     /* bin j = 4 + index, 375 j Hz: the sum of P_j over the n_segments segments */
} tfrec_amd_clock;
/* Turn the clock on: after tfrec_amd_enable_capture, before the first submit.  max_runs * 1056 bytes of device memory per FIFO set,
 * counted in tfrec_amd_get_memory.  Errors: no recorder, a second call, or a context of max_blocks >= 4096 (a record's spec is summed
 * on the device: below 2^15 segments it cannot overflow): TFREC_AMD_E_INVAL; after the first submit or a poisoned context:
 * TFREC_AMD_E_STATE; TFREC_AMD_E_NOMEM as elsewhere; a call that fails leaves the context exactly as it was.  A context on which it
 * was never called holds and launches what it did.  Independent of tfrec_amd_enable_burst_meter and tfrec_amd_enable_burst_envelope:
 * any subset.  Valid on every kind of context and in every mode, as the recorder is.  Its two kernels run on the recorder's
 * low-priority stream behind its own, the burst meter's and the envelope's. */
int tfrec_amd_enable_burst_clock(tfrec_amd_ctx *ctx);
/* out[i] = the record of entry i of the table tfrec_amd_read_captures returns for the same submit.  Conventions of tfrec_amd_read_bursts:
 * the OLDEST undrained submit, read BEFORE the drain that pops it; reading pops nothing; cap_runs is the room in records; *n_runs the
 * submit's true run count; out may be NULL with cap_runs 0 to fetch the count alone.  It reads the decimated samples, not the pool:
 * records are delivered for every entry below min(n_runs, max_runs), whatever max_samples is.  n_runs > max_runs:
 * TFREC_AMD_E_OVERFLOW with that prefix delivered.  Errors: not enabled, NULL ctx / n_runs / out (with cap_runs > 0), room too small
 * (nothing written, *n_runs set): TFREC_AMD_E_INVAL; nothing undrained or poisoned: TFREC_AMD_E_STATE. */
int tfrec_amd_read_burst_clocks(tfrec_amd_ctx *ctx, tfrec_amd_clock *out, size_t cap_runs, uint32_t *n_runs);

/* Burst track (tfrec_amd_enable_burst_track): for every run of the recorder's table what the burst SAID -- one bit per
 * captured sample, the sign of a quadrature discriminator about a centre frequency, boxcar-smoothed: 1 above the centre.  With the
 * rate from the burst clock and the centre from the burst meter a caller slices it into the burst's bits, at any rate, decoded or
 * not.  It sits on the recorder as the meter, the envelope and the clock do and is independent of them.  There is no reference
 * counterpart: this text is normative, tfrec_amd/track.py restates it.  Exact integers only.
 *   Settings: smooth = L, 1 .. 16, fixed at enable.  Per stream a centre hz, |hz| <= 192000, default 0
 *             (tfrec_amd_set_burst_track_centre); its table index r = floor((8192 hz + 384000) / 768000) mod 4096, a true floor for a
 *             negative hz too; C[], S[] are the tune table of tfrec_amd_tune_streams and no other.  A new centre takes effect with the
 *             next submit.  It is not a restart: a chain that spans the change is sliced with both, every product -- the carried ones
 *             included -- with the centre of the submit that forms it.
 *   Samples:  for entry e of a submit's table (tfrec_amd_run: stream s, submit-relative start a, n = n_samples, flags), z[k] = (I, Q),
 *             k = 0 .. n - 1, is the decimated pair at submit-relative index a + k, as for tfrec_amd_burst.  prior = the samples of the
 *             same chain ahead of this piece, held at 16: 0 without TFREC_AMD_RUN_CONTINUES, else min(16, prior' + n') of the OPEN
 *             piece (prior', n') that ended the submit before.
 *   Products: dot[k] = I[k] I[k-1] + Q[k] Q[k-1] and crs[k] = Q[k] I[k-1] - I[k] Q[k-1], the burst meter's products, in 64 bits;
 *             v[k] = crs[k] C[r] - dot[k] S[r], |v| < 2^47.  v[k] = 0 for the chain's first sample (k = 0 with prior = 0), and nothing
 *             ahead of the chain's first sample is ever used.  In a CONTINUES piece z[k] for -16 <= k < 0 are the stream's last 16
 *             pairs of the submit before, so the products of k - i < 0 are those of that submit's last samples.
 *   Track:    t[k] = 1 iff the sum of v[k - i] over 0 <= i < min(L, k + prior) is greater than 0 (no term: 0; a zero sum: 0); the
 *             sum stays below 2^51.
 *   Bits:     a bitmap of uint32 words: t[k] of entry e is bit (pool_offset_e + k) & 31 of word (pool_offset_e + k) >> 5, pool_offset
 *             the table entry's.  Bits that belong to no run, or to a run whose samples do not fit max_samples, are 0.
 *   Record:   the entry's first 24 bytes, bit_offset = its pool_offset, last_over = tfrec_amd_envelope's (the run-relative index of the
 *             run's last sample over the threshold in the final trigger mask, -1: none), n_ones = the number of k with t[k] = 1
 *             (counted whether or not the bits fit).
 *   Cutting:  a burst is a chain of pieces as for tfrec_amd_burst.  Merging concatenates the tracks, adds n_samples and n_ones, merges
 *             last_over by the envelope's rule (the last piece that has one, offset by the samples ahead of it), and takes the first
 *             piece's stream, start_sample, thresh and CONTINUES and the last piece's OPEN.  With one centre the merged record and
 *             track do not depend on how the stream was cut into submits.  A restart drops the chain.  tfrec_amd_save_streams does
 *             not carry the 16 pairs: a chain that continues behind tfrec_amd_load_streams uses what the context itself carried.
 *   Slicing (what a caller makes of a merged track; normative for tfrec_gpu -G and track.py): the input is the track's first
 *             last_over + 1 samples (none if -1) and a rate R in bit/s.  sym(l) = floor((2 l R + 384000) / 768000).  Walk the maximal
 *             runs (w, m) of equal track value w and length m in order, keeping (v, l): while nothing is kept a run with sym(m) == 0 is
 *             dropped and the first other run becomes (v, l); afterwards a run with sym(m) == 0 or w == v adds m to l, any other run
 *             emits sym(l) symbols of v and becomes (v, l); at the end sym(l) of v are emitted.  The bits are packed MSB-first.
 *             This is a discriminator and a run-length slicer, not a demodulator: it has no clock recovery, the five built-in
 *             decoders' filters are not applied, and a burst whose deviation is small against its carrier offset does not slice
 *             about the wrong centre.  Nothing of it has been measured on real recordings. */
typedef struct {            /* 40 bytes */
	uint32_t stream;        /* these five: copied from the table entry */
	uint32_t flags;
	int64_t  start_sample;
	uint32_t n_samples;
	int32_t  thresh;
	uint64_t bit_offset;    /* the entry's pool_offset: t[k] is bit bit_offset + k of the bitmap */
	int32_t  last_over;     /* as tfrec_amd_envelope's */
	uint32_t n_ones;        /* the number of k with t[k] = 1 */
} tfrec_amd_track;
/* Turn the track on: after tfrec_amd_enable_capture, before the first submit; smooth = L.  Device memory, counted in
 * tfrec_amd_get_memory: per FIFO set max_runs * 40 bytes, ceil(max_samples / 32) words and n_streams centre indices; per stream the
 * carried 16 pairs and prior (68 bytes); n_streams * 4 page-locked bytes per FIFO set.  Errors: smooth outside 1 .. 16, no recorder
 * or a second call: TFREC_AMD_E_INVAL; after the first submit or a poisoned context: TFREC_AMD_E_STATE; TFREC_AMD_E_NOMEM as
 * elsewhere; a call that fails leaves the context exactly as it was.  A context on which it was never called holds and launches
 * what it did.  Independent of the meter, the envelope and the clock: any subset.  Valid on every kind of context and in every
 * mode, as the recorder is, tfrec_amd_submit_runs included.  Its three kernels run on the recorder's low-priority stream behind
 * the others'. */
int tfrec_amd_enable_burst_track(tfrec_amd_ctx *ctx, int32_t smooth);
/* The centre of streams[i] becomes hz[i], from the next submit on (tfrec_amd_configure_streams' argument rules: n >= 0, both arrays
 * non-NULL when n > 0, every stream checked before anything is set).  |hz| > 192000, a stream out of range, or a context without
 * the track: TFREC_AMD_E_INVAL and nothing is set; a poisoned context: TFREC_AMD_E_STATE. */
int tfrec_amd_set_burst_track_centre(tfrec_amd_ctx *ctx, const int32_t *streams, const int32_t *hz, int n);
/* out[i] = the record of entry i of the table tfrec_amd_read_captures returns for the same submit, words = the bitmap.  The records
 * follow tfrec_amd_read_bursts' conventions (the OLDEST undrained submit, read BEFORE the drain that pops it; reading pops nothing;
 * out may be NULL with cap_runs 0; delivered for every entry below min(n_runs, max_runs)), the words tfrec_amd_read_captures' for the
 * pool: *n_words = ceil(delivered pairs / 32), the pairs being the submit's, or on an overflow those of the prefix of whole runs
 * the capture delivers; words may be NULL with cap_words 0, then none are copied.  More runs than max_runs or more pairs than
 * max_samples: TFREC_AMD_E_OVERFLOW with those prefixes delivered.  Errors: not enabled, NULL ctx / n_runs / n_words / out (with
 * cap_runs > 0) / words (with cap_words > 0), room too small (nothing written, the counts set): TFREC_AMD_E_INVAL; nothing undrained
 * or poisoned: TFREC_AMD_E_STATE. */
int tfrec_amd_read_burst_tracks(tfrec_amd_ctx *ctx, tfrec_amd_track *out, size_t cap_runs, uint32_t *n_runs, uint32_t *words,
				size_t cap_words, uint64_t *n_words);

/* Amplitude track (tfrec_amd_enable_burst_track_amplitude): a MODE of the burst track for on-off keyed bursts -- one
 * bit per captured sample, 1 where the burst's smoothed amplitude lies above a level.  A context has the frequency track above or the
 * amplitude track, never both.  The record (tfrec_amd_track), the bitmap's layout (Bits), last_over, n_ones and bit_offset (Record),
 * the merging rules (Cutting), the carry (the stream's last 16 pairs, and prior as under Samples), the overflow prefixes and
 * tfrec_amd_read_burst_tracks are exactly the frequency track's; so are the Slicing and everything the burst sync makes of a track.
 * Only the bit differs.  There is no reference counterpart: this text is normative, tfrec_amd/track.py (amplitude_tracks) restates
 * it.  Exact integers only.
 *   Settings: smooth = L, 1 .. 16, fixed at enable.  Per stream a level, 0 .. 65535, default 0 (tfrec_amd_set_burst_track_level), in
 *             the trigger's own unit: pwr = |I| + |Q| of a decimated pair, the unit of a stream's threshold and of tfrec_amd_burst's
 *             pwr_max.  A new level takes effect with the next submit.  It is not a restart: a chain that spans the change is sliced
 *             with both, every sum with the level of the submit that forms it.
 *   Bit:      for entry e with samples z[k] = (I, Q) and prior as for the frequency track, p[k] = |I| + |Q| (at most 65536).
 *             t[k] = 1 iff the sum of p[k - i] over the i with 0 <= i < L and k - i >= -prior is greater than L * level.  Samples
 *             ahead of the chain's first one count as 0 and are never read, so a burst's first L - 1 bits lean towards 0.  In a
 *             CONTINUES piece z[k] for -16 <= k < 0 are the stream's last 16 pairs of the submit before.  The sum stays below 2^21; a
 *             sum equal to L * level gives 0.  With one level and no TFREC_AMD_E_OVERFLOW the merged chain's track does not depend on
 *             how the stream was cut into submits.
 *   Pulses (what a caller makes of a merged track; normative for tfrec_gpu -O and track.py): take the track's first last_over + 1
 *             samples (none if -1) and the maximal runs of equal value in order; drop a leading run of zeros and a trailing run of
 *             zeros.  What remains alternates pulse width, gap width, ..., pulse width, in samples (nothing remains: no pulse).
 *             This is a level slicer with a level the caller gives, not an automatic gain control: a level too low reads the noise
 *             between pulses, one too high reads nothing.  Nothing of it has been measured on real recordings. */
/* Turn the track on in amplitude mode: tfrec_amd_enable_burst_track's rules, memory (the per-set values staged per stream are the
 * levels: the same bytes) and errors; a context whose track is on already, in either mode, refuses both enables with
 * TFREC_AMD_E_INVAL.  tfrec_amd_enable_burst_sync works on either mode.  One kernel differs on the recorder's stream. */
int tfrec_amd_enable_burst_track_amplitude(tfrec_amd_ctx *ctx, int32_t smooth);
/* The level of streams[i] becomes level[i], from the next submit on (tfrec_amd_set_burst_track_centre's argument rules).  A level
 * outside 0 .. 65535, a stream out of range, or a context whose track is off or in frequency mode: TFREC_AMD_E_INVAL and nothing is
 * set; a poisoned context: TFREC_AMD_E_STATE.  tfrec_amd_set_burst_track_centre on an amplitude context is TFREC_AMD_E_INVAL. */
int tfrec_amd_set_burst_track_level(tfrec_amd_ctx *ctx, const int32_t *streams, const int32_t *level, int n);

/* Auto-centre track (tfrec_amd_enable_burst_track_auto): a third MODE of the burst track, for a stream that holds the
 * bursts of several transmitters, each with its own carrier offset: every chain is tracked about a centre measured on its own first
 * samples, in the same submit, ahead of the track.  A context has the frequency track, the amplitude track or this one.  The record
 * (tfrec_amd_track), the bitmap, last_over, n_ones, the 16 carried pairs and prior, the merging rules, the overflow prefixes and
 * tfrec_amd_read_burst_tracks are exactly the frequency track's; so are the Slicing and everything the burst sync makes of a track.
 * Only the table index r that forms v[k] = crs[k] C[r] - dot[k] S[r] differs: it is the ENTRY's, not the stream's.  There is no
 * reference counterpart: this text is normative, tfrec_amd/track.py (head_centres, auto_tracks) restates it.  Exact integers only.
 *   Settings: fixed at enable: smooth = L, 1 .. 16, and head = K, 64 .. 4096 (K = 64 counts 63 products at the most and never
 *             measures).  Per stream the set centre hz, |hz| <= 192000, default 0 (tfrec_amd_set_burst_track_centre; in force from
 *             the next submit on): the FALLBACK.
 *   Counted:  for an entry without TFREC_AMD_RUN_CONTINUES, submit-relative start a and n samples, the products dot[k], crs[k] of the
 *             frequency track for 1 <= k < min(n, K); product k is counted iff over[a + k] and over[a + k - 1], over being the
 *             stream's final trigger mask, the one last_over is taken from.  Both pairs are then over a threshold >= 0, so neither is
 *             (0, 0) and the product is not.  The head is read from the decimated samples, not from the pool: max_samples does not
 *             matter to it.
 *   Centre:   P = the number of counted products, hist[j] their count in bin j of tfrec_amd_burst's 64 bins of 6 kHz.  If P >= 64, bin
 *             j is occupied iff hist[j] >= floor((P + 15) / 16); lo and hi are the smallest and the largest SIGNED index (j for
 *             j < 32, j - 64 otherwise) of an occupied bin.  With an occupied bin: centre_hz = 3000 (lo + hi), deviation_hz =
 *             3000 (hi - lo), source MEASURED.  With P < 64, or with no occupied bin (products spread so thinly that no bin holds
 *             a sixteenth of them: noise): centre_hz = the stream's set centre, deviation_hz = 0, source FALLBACK.  n_counted = P in
 *             both.  r = floor((8192 centre_hz + 384000) / 768000) mod 4096, as for the frequency track.
 *   Chains:   an entry with TFREC_AMD_RUN_CONTINUES takes r and centre_hz of the OPEN entry that ended the submit before: source
 *             INHERITED, n_counted = deviation_hz = 0.  Where that entry had no record (it lay beyond max_runs) the set centre is
 *             used, source FALLBACK.  A restart needs nothing: the run behind it does not CONTINUE and is measured as a chain's
 *             first piece.  tfrec_amd_save_streams does not carry the centre.
 *   Limits:   the chain's first piece decides for the whole chain.  The merged track therefore does not depend on the cut whenever
 *             the chain's first piece holds at least min(n_chain, K) samples; a chain that begins within K samples of a submit's
 *             end is centred on what its first piece has (fewer than 65 samples: the fallback).  The histogram is not circular: a
 *             burst whose |centre| + deviation approaches 192 kHz wraps around and reads wrongly.  Nothing of it has been measured on
 *             real recordings.
 *   Cutting:  merging a chain keeps the first piece's centre record and gives it the merged flags and n_samples of tfrec_amd_track. */
#define TFREC_AMD_CENTRE_MEASURED 0u
#define TFREC_AMD_CENTRE_FALLBACK 1u
#define TFREC_AMD_CENTRE_INHERITED 2u
typedef struct {            /* 48 bytes */
	uint32_t stream;        /* these five: copied from the table entry */
	uint32_t flags;
	int64_t  start_sample;
	uint32_t n_samples;
	int32_t  thresh;
	uint32_t n_counted;     /* P */
	uint32_t source;        /* TFREC_AMD_CENTRE_* */
	int32_t  centre_hz;     /* the one the entry's track is formed about */
	int32_t  deviation_hz;  /* of a measured centre, else 0 */
	int32_t  index;         /* r */
	uint32_t reserved;      /* 0 */
} tfrec_amd_track_centre;
/* Turn the track on in auto-centre mode: tfrec_amd_enable_burst_track's rules and errors, and head outside 64 .. 4096:
 * TFREC_AMD_E_INVAL; a context whose track is on already, in any mode, refuses all three enables with TFREC_AMD_E_INVAL.  Memory: the
 * frequency track's (the per-set values staged per stream are the set centres in Hz: the same bytes), and per FIFO set max_runs * 48
 * bytes, per stream the carried index and centre (8 bytes).  tfrec_amd_set_burst_track_centre sets the fallback;
 * tfrec_amd_set_burst_track_level is TFREC_AMD_E_INVAL.  tfrec_amd_enable_burst_sync works on this mode too.  Six launches on the
 * recorder's stream: both records' inits, the head's histogram and resolve, the track about every entry's index, the two carries. */
int tfrec_amd_enable_burst_track_auto(tfrec_amd_ctx *ctx, int32_t smooth, int32_t head);
/* out[i] = the centre record of entry i of the table tfrec_amd_read_captures returns for the same submit: tfrec_amd_read_bursts'
 * conventions, counts, prefix on TFREC_AMD_E_OVERFLOW (records for every entry below min(n_runs, max_runs), whatever max_samples
 * is) and errors; a context whose track is off or in another mode: TFREC_AMD_E_INVAL. */
int tfrec_amd_read_burst_track_centres(tfrec_amd_ctx *ctx, tfrec_amd_track_centre *out, size_t cap_runs, uint32_t *n_runs);

/* Phase track (tfrec_amd_enable_burst_track_phase): a fourth MODE of the burst track, for PHASE-keyed bursts, whose
 * frequency does not move and on which a discriminator has nothing to read: a differential phase detector at a lag of m samples -- a
 * symbol -- about the burst's own carrier, measured on the chain's first samples in the same submit.  A context has the frequency
 * track, the amplitude track, the auto-centre track or this one.  The record (tfrec_amd_track), the bitmap and its packing, last_over,
 * n_ones, the merging rules, the overflow prefixes, tfrec_amd_read_burst_tracks, and tfrec_amd_read_burst_track_centres with
 * tfrec_amd_track_centre and its three sources are exactly the frequency track's and the auto-centre track's; so are the Slicing and
 * everything the burst sync makes of a track.  There is no reference counterpart: this text is normative, tfrec_amd/track.py
 * (head_carriers, phase_tracks) restates it.  Exact integers only.
 *   Settings: fixed at enable: smooth = L, 1 .. 16, the detector's boxcar; head = K, 64 .. 4096, the samples of a chain's first piece
 *             the carrier is measured on (K = 64 counts 63 products at the most and never measures); lag = m, 1 .. 64, the
 *             detector's lag in samples.  Per stream the set centre hz, |hz| <= 192000, default 0
 *             (tfrec_amd_set_burst_track_centre; in force from the next submit on): the FALLBACK.
 *   Carrier:  for an entry without TFREC_AMD_RUN_CONTINUES, submit-relative start a and n samples, the counted products are the
 *             auto-centre track's: dot[k], crs[k] of the frequency track for 1 <= k < min(n, K), counted iff over[a + k] and
 *             over[a + k - 1] in the stream's final trigger mask.  P is their number, A the sum of dot over them and B the sum of
 *             crs: |dot|, |crs| <= 2^31 and P <= 4095, so |A|, |B| < 2^43.  With C[], S[] the tune table (C[r] = round(32767 cos(2 pi
 *             r / 4096)), S[r] = C[(r - 1024) mod 4096]), score(r) = A C[r] + B S[r] and cross(r) = B C[r] - A S[r]; both stay below
 *             2^59.  If P >= 64 and (A, B) != (0, 0): r is the index in 0 .. 4095 with score(r) > 0 that minimises |cross(r)|, on a
 *             tie the smallest such index (one exists: the index nearest the direction of (A, B) has a positive score); source
 *             MEASURED, centre_hz = floor(375 rs / 4) with rs = r below 2048 and r - 4096 otherwise, deviation_hz = 0.  The zero of
 *             the cross term, not the maximum of the score: near its peak the score changes per index by about a tenth of the
 *             table's rounding, the cross term by about 50 times its rounding.  Otherwise r = floor((8192 hz + 384000) / 768000) mod
 *             4096 of the stream's set centre hz, centre_hz = hz, deviation_hz = 0, source FALLBACK.  n_counted = P in both.
 *   Chains:   an entry with TFREC_AMD_RUN_CONTINUES is exactly the auto-centre track's: INHERITED from the OPEN entry that ended the
 *             submit before, or FALLBACK where that entry had no record; n_counted = deviation_hz = 0.
 *   Products: rm = (r m) mod 4096.  c(k) is sample k's index in its chain, counted from the chain's first sample (k + prior in an
 *             entry that CONTINUES, k otherwise, k being run-relative).  For c(k) >= m: dm = I[k] I[k-m] + Q[k] Q[k-m], cm = Q[k]
 *             I[k-m] - I[k] Q[k-m], u[k] = dm C[rm] + cm S[rm]: the real part of z[k] conj(z[k-m]) turned back by the carrier's
 *             advance over m samples; |u| < 2^47.  u[k] = 0 for c(k) < m: nothing ahead of the chain is ever used.
 *   Track:    t[k] = 1 iff the sum of u[k - i] over 0 <= i < L is greater than 0, terms ahead of the chain counting as 0; a zero sum
 *             gives 0.  1: the same phase as m samples ago.  For an NRZ-S signal -- the carrier toggles on every 0 bit -- with m
 *             one symbol that is the data bit itself.
 *   Carried:  per stream the last 80 pairs of the submit and prior = min(80, prior' + n') of its OPEN piece.  80 = 64 + 16: t[k] of
 *             a piece's first sample (k = 0) sums u[-i] for i <= L - 1 <= 15, u[-i] reads z[-i - m] with m <= 64: 79 pairs back
 *             at the most, and c(k) >= m is decided alike by prior and by min(80, prior) since k - i + 80 >= 65 > m.  Also, as in
 *             the auto-centre track, the index and centre of the run that reaches the submit's end.  tfrec_amd_save_streams carries
 *             none of it.
 *   Cutting:  the merged track is the uncut run's whenever the chain's first piece holds at least min(n_chain, K) samples; a chain
 *             that begins within K samples of a submit's end is read about what its first piece has (fewer than 65 samples: the
 *             fallback).  Merging a chain keeps the first piece's centre record.
 *   Limits:   the carrier is the direction of the SUM of the head's one-sample products: a signal whose products cancel (a phase
 *             that flips by a half turn every sample) has no carrier this way and falls back.  The detector reads a symbol
 *             against the one before it; m must be the symbol's length to within the boxcar.  No descrambler, no bit order: a
 *             caller makes bytes of the bits.  Nothing of it has been measured on real recordings. */
/* Turn the track on in phase mode: tfrec_amd_enable_burst_track_auto's rules and errors, and lag outside 1 .. 64: TFREC_AMD_E_INVAL; a
 * context whose track is on already, in any mode, refuses all four enables with TFREC_AMD_E_INVAL.  Memory: the auto-centre track's
 * with 80 carried pairs per stream in the place of its 16 (320 bytes for 64).  tfrec_amd_set_burst_track_centre sets the fallback;
 * tfrec_amd_set_burst_track_level is TFREC_AMD_E_INVAL.  tfrec_amd_enable_burst_sync works on this mode too.  Six launches on the
 * recorder's stream: both records' inits, the head's carrier, the detector about every entry's index, the two carries. */
int tfrec_amd_enable_burst_track_phase(tfrec_amd_ctx *ctx, int32_t smooth, int32_t head, int32_t lag);

/* Burst sync (tfrec_amd_enable_burst_sync): for every run of the recorder's table WHERE A FRAME BEGINS -- one bit per
 * captured sample, 1 where the burst track, read at P symbol centres that end at the sample, is a known sync word but for at most E
 * places.  The symbol timing comes from where the matches lie; a caller reads the payload at symbol centres from there.  It sits on
 * the burst track and needs it.  There is no reference counterpart: this text is normative, tfrec_amd/sync.py restates it.  Exact
 * integers only.
 *   Settings: fixed at enable.  A rate R in bit/s, 1000 .. 96000; a pattern, the low P bits of a uint64, 8 <= P <= 64, the most
 *             significant of them transmitted first: pattern bit j, j = 0 .. P - 1, is (pattern >> j) & 1, and bit 0 is the LAST one
 *             transmitted; E with 0 <= E and 2 E < P; the flag TFREC_AMD_SYNC_BOTH.  delta(i) = floor((768000 i + R) / (2 R)), the
 *             samples from a symbol's centre to the centre i symbols on (delta(0) = 0); span = delta(P - 1) <= 2047.
 *   History:  for entry e of a submit's table with track t[0 .. n) (tfrec_amd_track), t[-1], t[-2], ... are the track bits of the
 *             same chain ahead of this piece, of which H are available: H = 0 without TFREC_AMD_RUN_CONTINUES, else H =
 *             min(2047, H' + n') of the OPEN piece (H', n') that ended the submit before.  Per stream the device carries the last
 *             2047 track bits of the chain of its OPEN run and H; a piece shorter than 2047 samples that continues a chain combines
 *             what was carried with its own bits.
 *   Distance: for k + H >= span, d[k] = the number of j in 0 .. P - 1 with t[k - delta(j)] != pattern bit j (bit 0 sits at k
 *             itself); otherwise d[k] is undefined.
 *   Match:    m[k] = 1 iff d[k] is defined and (d[k] <= E, or TFREC_AMD_SYNC_BOTH and d[k] >= P - E: the complemented word).
 *   Bits:     packed exactly as the track's: m[k] of entry e is bit (pool_offset_e + k) & 31 of word (pool_offset_e + k) >> 5.  Bits
 *             that belong to no run are 0.  A run whose samples do not fit max_samples is not looked at: its bits are 0, its n_hits
 *             0, its best 0xffffffff, and it leaves H = 0 behind it, so that its continuation starts without history; so does an
 *             OPEN run beyond max_runs, which has no record.  The independence of the cut (below) is therefore claimed only for
 *             submits without TFREC_AMD_E_OVERFLOW.
 *   Record:   the entry's first 24 bytes, bit_offset = its pool_offset, n_hits = the number of k with m[k] = 1, best = the minimum of
 *             d[k] over the defined k -- with TFREC_AMD_SYNC_BOTH of min(d[k], P - d[k]) -- or 0xffffffff where no k is defined,
 *             best_at = the first k that has it (0 where none), and a reserved word, 0.
 *   Cutting:  a burst is a chain of pieces as for tfrec_amd_burst.  Merging concatenates the match tracks, adds n_samples and
 *             n_hits, takes the smaller best -- on a tie the earlier piece's -- with its best_at offset by the samples ahead of
 *             its piece, and the flags as for tfrec_amd_track.  With one track centre and no overflow the merged record and match
 *             track do not depend on how the stream was cut into submits.  A restart needs nothing: only a CONTINUES run reads what
 *             was carried.  tfrec_amd_save_streams does not carry the history: a chain that continues behind
 *             tfrec_amd_load_streams uses what the context itself carried.
 *   Framing (what a caller makes of a chain's merged track and match track; normative for tfrec_gpu -Y and sync.py): the input is
 *             the first last_over + 1 samples of both (last_over: the merged tfrec_amd_track's), of the first 2^20 at most.  The
 *             plateaus are the maximal runs [a, b] of ones in m; a plateau's sample is c = (a + b) >> 1.  For each plateau, in
 *             order, d[c] is counted again on the merged track, a track bit ahead of its first one reading 0: the polarity is +
 *             if d[c] <= E, else -, and the errors are d[c] or P - d[c] accordingly.  The payload is the track's bits at
 *             c + delta(i) for i = 1, 2, ... (delta by the same formula beyond P - 1) up to the number of bits wanted; it stops at
 *             the first position outside the input, and is complemented under -.  It is packed MSB-first.
 * Nothing of it has been measured on real recordings. */
#define TFREC_AMD_SYNC_BOTH 1u  /* tfrec_amd_enable_burst_sync's flag: the complemented pattern matches too */
typedef struct {            /* 48 bytes */
	uint32_t stream;        /* these five: copied from the table entry */
	uint32_t flags;
	int64_t  start_sample;
	uint32_t n_samples;
	int32_t  thresh;
	uint64_t bit_offset;    /* the entry's pool_offset: m[k] is bit bit_offset + k of the bitmap */
	uint32_t n_hits;        /* the number of k with m[k] = 1 */
	uint32_t best;          /* the smallest distance; 0xffffffff: none defined */
	uint32_t best_at;       /* the first k that has it */
	uint32_t reserved;      /* 0 */
} tfrec_amd_burst_sync;
/* Turn the sync on: after tfrec_amd_enable_burst_track, before the first submit, once.  pattern: its low n_bits bits (higher ones
 * are ignored); flags: 0 or TFREC_AMD_SYNC_BOTH.  Device memory, counted in tfrec_amd_get_memory: per FIFO set max_runs * 48 bytes
 * and ceil(max_samples / 32) words; per stream the carried 64 words and H (260 bytes); no page-locked memory.  Errors: a rate
 * outside 1000 .. 96000, n_bits outside 8 .. 64, max_errors < 0 or 2 max_errors >= n_bits, an unknown flag, a span above 2047, no
 * burst track or a second call: TFREC_AMD_E_INVAL; after the first submit or a poisoned context: TFREC_AMD_E_STATE;
 * TFREC_AMD_E_NOMEM as elsewhere; a call that fails leaves the context exactly as it was.  A context on which it was never called
 * holds and launches what it did.  Its three kernels run on the recorder's low-priority stream behind the track's. */
int tfrec_amd_enable_burst_sync(tfrec_amd_ctx *ctx, int32_t rate, uint64_t pattern, int32_t n_bits, int32_t max_errors, uint32_t flags);
/* out[i] = the record of entry i of the table tfrec_amd_read_captures returns for the same submit, words = the match bitmap:
 * tfrec_amd_read_burst_tracks' conventions, counts, prefixes on TFREC_AMD_E_OVERFLOW and errors throughout. */
int tfrec_amd_read_burst_syncs(tfrec_amd_ctx *ctx, tfrec_amd_burst_sync *out, size_t cap_runs, uint32_t *n_runs, uint32_t *words,
			       size_t cap_words, uint64_t *n_words);

/* Line code (tfrec_amd_enable_burst_code): an optional stage of the burst track, valid in any of its four modes, for
 * transmitters whose bits are differentially coded (NRZI, NRZ-S) or scrambled by a self-synchronising scrambler (G3RUH) on the air: a
 * sync word that exists only behind the line decoder is never found on the raw track.  Such a decoder is an XOR of the track with
 * copies of itself delayed by whole symbols, so its output has the track's shape: one bit per captured sample.  With the code on,
 * tfrec_amd_enable_burst_sync correlates the CODED track, and its own carried history holds coded bits.  There is no reference
 * counterpart: this text is normative, tfrec_amd/linecode.py restates it.  Exact integers only.
 *   Settings: fixed at enable.  A rate R in bit/s, 1000 .. 96000; taps, a non-zero uint32: bit j - 1 set means a delay of j symbols,
 *             j = 1 .. 32; the flag TFREC_AMD_CODE_INVERT.  delta(j) = floor((768000 j + R) / (2 R)), the burst sync's delta;
 *             span = delta(the highest set tap) <= 2047.  G3RUH (1 + x^12 + x^17) is taps 0x10800, NRZI taps 1, NRZ-S taps 1 with
 *             INVERT.
 *   History:  for entry e of a submit's table with track t[0 .. n) (tfrec_amd_track), t[x] for x < 0 is the track bit of the same
 *             chain ahead of this piece, where the chain has one.  H of them are available: H = 0 without TFREC_AMD_RUN_CONTINUES,
 *             else H = min(2047, H' + n') of the OPEN piece (H', n') that ended the submit before; H < 2047 is the whole chain so
 *             far.  t[x] = 0 for x < -H: ahead of the chain's first sample.  Per stream the device carries the last 2047 track bits
 *             of the chain of its OPEN run and H, separately from the burst sync's.
 *   Bit:      u[k] = t[k] ^ (the XOR over the set taps j of t[k - delta(j)]) ^ invert, for 0 <= k < n; invert is 1 under
 *             TFREC_AMD_CODE_INVERT, which therefore also complements what the bits ahead of the chain contribute (0 ^ 1).
 *   Bits:     packed exactly as the track's: u[k] of entry e is bit (pool_offset_e + k) & 31 of word (pool_offset_e + k) >> 5.  Bits
 *             that belong to no run are 0.  A run whose samples do not fit max_samples has no track: its bits are 0, its n_ones 0,
 *             and it leaves H = 0 behind it; so does an OPEN run beyond max_runs, which has no record.  The independence of the cut
 *             is therefore claimed only for submits without TFREC_AMD_E_OVERFLOW.
 *   Record:   a tfrec_amd_track: the entry's first 24 bytes, bit_offset = its pool_offset, last_over = the track record's of the same
 *             entry, n_ones = the number of k with u[k] = 1.  The track's merging rules, its Slicing and the burst sync's Framing
 *             work on it unchanged.
 *   Cutting:  with one track centre and no overflow the merged record and coded track do not depend on how the stream was cut into
 *             submits.  A restart drops the chain: the run behind it does not CONTINUE.  tfrec_amd_save_streams does not carry the
 *             history: a chain that continues behind tfrec_amd_load_streams uses what the context itself carried.
 * No CRC of its own (see the frame check below), no Manchester decoding, no additive (frame-synchronous) scrambler.  Nothing of it has been measured on real recordings. */
#define TFREC_AMD_CODE_INVERT 1u  /* tfrec_amd_enable_burst_code's flag: the coded bit is complemented */
/* Turn the line code on: after tfrec_amd_enable_burst_track (any mode), before the first submit, once; before or after
 * tfrec_amd_enable_burst_sync.  Device memory, counted in tfrec_amd_get_memory: per FIFO set max_runs * 40 bytes and
 * ceil(max_samples / 32) words; per stream the carried 64 words and H (260 bytes); no page-locked memory.  Errors: a rate outside
 * 1000 .. 96000, taps == 0, an unknown flag, a span above 2047, no burst track or a second call: TFREC_AMD_E_INVAL, and nothing is
 * allocated; after the first submit or a poisoned context: TFREC_AMD_E_STATE; TFREC_AMD_E_NOMEM as elsewhere; a call that fails
 * leaves the context exactly as it was.  A context on which it was never called holds and launches what it did.  Valid wherever the
 * recorder is, tfrec_amd_submit_runs included.  Its three kernels run on the recorder's low-priority stream behind the track's and
 * ahead of the sync's. */
int tfrec_amd_enable_burst_code(tfrec_amd_ctx *ctx, int32_t rate, uint32_t taps, uint32_t flags);
/* out[i] = the coded record of entry i of the table tfrec_amd_read_captures returns for the same submit, words = the coded bitmap:
 * tfrec_amd_read_burst_tracks' conventions, counts, prefixes on TFREC_AMD_E_OVERFLOW and errors throughout. */
int tfrec_amd_read_burst_codes(tfrec_amd_ctx *ctx, tfrec_amd_track *out, size_t cap_runs, uint32_t *n_runs, uint32_t *words,
			       size_t cap_words, uint64_t *n_words);

/* Frame check (tfrec_amd_enable_burst_crc): an optional stage of the burst track, valid in any of its four modes: for
 * every run of the recorder's table WHERE A FRAME THAT CARRIES ITS OWN CRC ENDS -- one bit per captured sample, 1 where the N bytes
 * whose last bit sits at the sample, read at the Framing's symbol centres, check.  Its input track t is the coded bitmap where
 * tfrec_amd_enable_burst_code is on, else the track's -- the burst sync's input; the choice is made per submit, so the enables may
 * come in any order.  It needs no sync: it finds frames behind a sync word nobody knows.  There is no reference counterpart: this
 * text is normative, tfrec_amd/crc.py restates it.  Exact integers only.
 *   Settings: fixed at enable.  A rate R in bit/s, 1000 .. 96000; n_bytes = N, 1 .. 256, the frame behind the sync word: skipped
 *             bytes, covered bytes and the CRC field; skip = S >= 0; width = W, one of 8, 16, 24, 32; S + W / 8 < N (at least one
 *             covered byte); poly non-zero; poly, init and xorout below 2^W; the flags TFREC_AMD_CRC_LSB (a byte's first received bit
 *             is its bit 0; otherwise its bit 7) and TFREC_AMD_CRC_INVERT (every bit is complemented before use).  delta(i) =
 *             floor((768000 i + R) / (2 R)), the burst sync's; D = delta(8 N) <= 16383.  At 6001 bit/s N = 32 gives D = 16381; at 6000
 *             it gives 16384 and is refused.
 *   Bits:     for sample k of an entry, b_i = t[k - (D - delta(i))] ^ invert, i = 1 .. 8 N; b_{8N} sits at k itself.  These are the
 *             Framing's payload positions for a sync centre c = k - D.  Byte j, j = 0 .. N - 1, is assembled from b_{8j+1} .. b_{8j+8}
 *             in the flag's order.
 *   CRC:      with no reflection: r = init; for each covered byte j, S <= j < N - W / 8: r ^= byte << (W - 8), then eight times r =
 *             ((r << 1) ^ poly if r's top bit was set, else r << 1) mod 2^W.  field = the last W / 8 bytes, big-endian.
 *             v[k] = 1 iff k + H >= D and (r ^ xorout) == field.
 *   History:  the burst sync's with a longer reach: H = 0 without TFREC_AMD_RUN_CONTINUES, else H = min(16383, H' + n') of the OPEN
 *             piece (H', n') that ended the submit before.  Per stream the device carries the chain's last 16384 input-track bits
 *             (512 words) and H, its own, separate from the sync's and the code's.  A sample with k + H < D is undefined and reads 0,
 *             so bits ahead of the chain's first sample are never used and stale carried words cannot matter.  A run that does not
 *             fit max_samples, or an OPEN run beyond max_runs: bits 0, n_ok 0, first_at none, and H = 0 behind it; the independence
 *             of the cut is claimed without TFREC_AMD_E_OVERFLOW only.  A reset drops the chain: the run behind it does not
 *             CONTINUE.  tfrec_amd_save_streams does not carry the history.
 *   Bits of v: packed exactly as the track's, at the entry's pool_offset.  Bits that belong to no run are 0.
 *   Record:   the entry's first 24 bytes, bit_offset = its pool_offset, n_ok = the number of k with v[k] = 1, first_at = the first
 *             such k, or 0xffffffff where there is none.
 *   Merging:  the v tracks are concatenated, n_samples and n_ok added; first_at is that of the first piece that has one, offset by
 *             the samples ahead of that piece; the flags as for tfrec_amd_track.  Without overflow the merged record and check track
 *             do not depend on how the stream was cut into submits.
 *   Verdict   (an addition to the burst sync's Framing; normative for tfrec_gpu -V and crc.py): a frame of polarity + with all 8 N
 *             payload bits is ok iff v[c + D] = 1 on the merged check track, else bad; c + D = c + delta(8 N) is the position of its
 *             last bit and lies inside the input.  A frame with fewer bits has no verdict.  tfrec_gpu keeps the first 2^20 samples
 *             of a chain's tracks (the Framing's input): a frame whose last bit lies behind them has no verdict there ("-"), and
 *             a piece that a file's end cuts has n_ok and first_at counted again on what is kept; crc.py has no such limit.
 *   Limits:   one N per context (TX22's telegrams of 7 and 9 bytes need two).  Reflected CRCs, the complemented reading under
 *             TFREC_AMD_SYNC_BOTH and frames whose length a byte of the frame gives are out of scope; the complement only changes
 *             the constant the residue starts from.  With init = 0 and xorout = 0 an all-zero frame checks, so a burst's constant
 *             stretches raise n_ok: n_ok alone is a detector only for CRCs with a non-zero init.  Nothing of it has been measured
 *             on real recordings. */
#define TFREC_AMD_CRC_LSB 1u     /* tfrec_amd_enable_burst_crc's flags: a byte's first received bit is its bit 0 */
#define TFREC_AMD_CRC_INVERT 2u  /* ... every input bit is complemented before use */
typedef struct {            /* 40 bytes */
	uint32_t stream;        /* these five: copied from the table entry */
	uint32_t flags;
	int64_t  start_sample;
	uint32_t n_samples;
	int32_t  thresh;
	uint64_t bit_offset;    /* the entry's pool_offset: v[k] is bit bit_offset + k of the bitmap */
	uint32_t n_ok;          /* the number of k with v[k] = 1 */
	uint32_t first_at;      /* the first such k; 0xffffffff: none */
} tfrec_amd_burst_crc;
/* Turn the frame check on: after tfrec_amd_enable_burst_track (any mode), before the first submit, once; before or after
 * tfrec_amd_enable_burst_code and tfrec_amd_enable_burst_sync, and without them.  Device memory, counted in tfrec_amd_get_memory: per
 * FIFO set max_runs * 40 bytes and ceil(max_samples / 32) words; per stream the carried 512 words and H (2052 bytes); once, the term
 * table, 8 n_bytes terms of 8 bytes; no page-locked memory.  Errors: any setting outside the above, an unknown flag, D > 16383, no
 * burst track or a second call: TFREC_AMD_E_INVAL, and nothing is allocated; after the first submit or a poisoned context:
 * TFREC_AMD_E_STATE; TFREC_AMD_E_NOMEM as elsewhere; a call that fails leaves the context exactly as it was.  A context on which it
 * was never called holds and launches what it did.  Valid wherever the recorder is, tfrec_amd_submit_runs included.  Its three
 * kernels run on the recorder's low-priority stream behind the line code's (or the track's). */
int tfrec_amd_enable_burst_crc(tfrec_amd_ctx *ctx, int32_t rate, int32_t n_bytes, int32_t skip, int32_t width, uint32_t poly, uint32_t init,
			       uint32_t xorout, uint32_t flags);
/* out[i] = the record of entry i of the table tfrec_amd_read_captures returns for the same submit, words = the check bitmap:
 * tfrec_amd_read_burst_tracks' conventions, counts, prefixes on TFREC_AMD_E_OVERFLOW and errors throughout. */
int tfrec_amd_read_burst_crcs(tfrec_amd_ctx *ctx, tfrec_amd_burst_crc *out, size_t cap_runs, uint32_t *n_runs, uint32_t *words,
			      size_t cap_words, uint64_t *n_words);

/* Power spectrum of the input rows (tfrec_amd_enable_spectrum): where in a recording there is energy, and where the
 * short bursts are that an average hides -- before a receiver is placed.  It belongs to an input ROW of a submit, not to a stream: it
 * is taken on x, the int16 value every format maps a stored component to (tfrec_amd_create_format; -8192 <= x <= 8191), at the
 * context's input rate, ahead of every tune, resampler and FIR.  Valid on every kind of context (tfrec_amd_create,
 * TFREC_AMD_F_INPUT_10X, rate and format contexts).  Exact integers only: a direct DFT with one rounding before it and one after it
 * and nothing in between, so that the order of summation cannot matter.  No reference counterpart; pinned by tfrec_amd/spectrum.py.
 *   Tables:  C[k] = round(32767 * cos(2 pi k / 4096)), S[k] = C[(k - 1024) mod 4096] -- tfrec_amd_tune_streams' table, no other.
 *            N = n_bins, one of 64, 128, 256, 512, 1024;  step = 4096 / N.
 *   Window:  w[n] = (32767 - C[(n * step) mod 4096]) >> 1,  n = 0 .. N-1  (periodic Hann; 0 <= w <= 32767, w[0] = 0, w[N/2] = 32767).
 *   Sample:  xw = (x * w[n] + 2^14) >> 15  per rail (int32, arithmetic shift): |xw| <= 8192.
 *   Frames:  frame f of a submit covers the row's input samples [f N, (f + 1) N), counted from the submit's first sample;
 *            F = floor(n_in / N) frames, n_in = the submit's complex samples per row (tfrec_amd_input_bytes / bytes per sample).  A
 *            tail shorter than N is not analysed.  Nothing is carried from submit to submit; a restart of a stream does not touch it.
 *   DFT:     for bin k = 0 .. N-1 and t = (k * n * step) mod 4096:
 *                X_re[k] = sum_n ( xwI * C[t] + xwQ * S[t] ),   X_im[k] = sum_n ( xwQ * C[t] - xwI * S[t] )
 *            The sign is the mixer's: a tone at +f lands in bin round(f N / fs_in), one at -f in bin N - that.  Exact integers: a term
 *            is at most 8192 * (|C[t]| + |S[t]|) <= 8192 * 46341 < 2^29 in magnitude, so |X| < 2^39 at N = 1024, and every partial sum
 *            of every grouping stays far below 2^53: int64 -- or fp64 on these integer operands -- is exact in any order.
 *   Power:   Y = (X + 2^14) >> 15 per component (arithmetic shift), p[k] = Y_re^2 + Y_im^2  (|Y| < 2^24, p < 2^49).
 *   Records: G = frames_per_record consecutive frames form a record: record r of a submit holds frames [r G, min((r + 1) G, F)),
 *            ceil(F / G) records, the last may be short.  Per record and bin: sum[k] = sum of p[k] over its frames (< 2^63),
 *            peak[k] = the largest p[k] among them (the peak hold that keeps a 10 ms burst visible in a one-second record); per
 *            record n_frames, the frames it holds.
 *   Cutting: where N divides every submit's n_in and G every submit's F, the concatenated records do not depend on how the input is
 *            cut into submits; otherwise they do (frames and records are counted from each submit's first sample).
 * tfrec_amd_enable_spectrum: allowed only before the first submit (after it: TFREC_AMD_E_STATE).  Rows 0 .. min(R, max_rows) - 1 of
 * each submit are analysed, R = the rows the submit provides (tfrec_amd_map_streams: 1 + the highest row a stream reads; n_streams
 * on an unmapped context).  Per FIFO set (TFREC_AMD_FIFO_DEPTH of them) it allocates max_rows * max_records * N * 16 bytes for
 * sums and peaks and max_rows * max_records * 4 bytes for the frame counts, max_records = ceil(floor(n_max / N) / G) with n_max =
 * floor(max_blocks * 32768 * P / Q) (the context's input rate P / Q; 10 / 1 with TFREC_AMD_F_INPUT_10X); tfrec_amd_get_memory counts
 * all of it.  The one kernel runs on a low-priority stream of its own, ordered behind the producer of the input only; events,
 * levels and captures do not depend on it.
 * Errors: n_bins outside the list, frames_per_record outside [1, 16384], max_rows outside [1, n_streams], a NULL context or a
 * second call: TFREC_AMD_E_INVAL; TFREC_AMD_E_NOMEM leaves the context usable without the spectrum (and holding nothing for it); a
 * poisoned context: TFREC_AMD_E_STATE.  A call that fails leaves the context exactly as it was before it: tfrec_amd_get_memory
 * reports what it reported, and a later call is a first one.
 * A context on which it was never called creates no stream, event or buffer for this and launches what it launched before. */
int tfrec_amd_enable_spectrum(tfrec_amd_ctx *ctx, int32_t n_bins, int32_t frames_per_record, int32_t max_rows);
/* The spectrum records of one input row of the OLDEST undrained submit (waits for it; like tfrec_amd_read_levels, call it BEFORE
 * tfrec_amd_drain_events pops that submit; reading pops nothing): sum[r * N + k], peak[r * N + k], n_frames[r] for r < *n_records;
 * cap_records is the room in records.  sum, peak and n_frames may be NULL with cap_records 0 to fetch only *n_records.
 * Errors: the spectrum not enabled, a row the submit's spectrum does not cover (row < 0 or row >= min(R, max_rows)), n_records
 * NULL: TFREC_AMD_E_INVAL; the room too small (or a NULL array with records to deliver): TFREC_AMD_E_INVAL, nothing is written, but
 * *n_records is set; nothing undrained or a poisoned context: TFREC_AMD_E_STATE. */
int tfrec_amd_read_spectrum(tfrec_amd_ctx *ctx, int32_t row, uint64_t *sum, uint64_t *peak, size_t cap_records, uint32_t *n_frames,
			    int *n_records);

/* Occupancy detector (tfrec_amd_enable_occupancy): which bins of a spectrum record hold a signal -- decided on the
 * device, on the records of the spectrum above while they lie in device memory, so that a caller who only wants to know where the
 * channels are reads 16 + N / 8 bytes per record instead of 16 N.  It sits on top of the spectrum: tfrec_amd_enable_spectrum comes
 * first, and records, rows and the cutting rule are the spectrum's, unchanged.  Exact integers only, on a record's sum[k], peak[k]
 * and n_frames with N = n_bins; no tolerance, no floating point.  No reference counterpart; pinned by tfrec_amd/occupancy.py.
 *   Parameters: ratio within [2, 4096], rel within [1, 4096].
 *   Mean:    m[k] = sum[k] / n_frames  (floor division of uint64; < 2^49).
 *   Floor:   the LOWER MEDIAN of m: with the N values of m sorted ascending, the value at index N / 2 - 1.  A value, not a
 *            position: ties cannot matter.
 *   Top:     top = max over k of peak[k].
 *   Hit:     hit[k] = peak[k] > max(floor, 1) * ratio  AND  peak[k] * rel >= top.  peak < 2^49 and the factors are at most 2^12:
 *            both products stay below 2^61.  max(floor, 1) keeps a record whose median is 0 from hitting wherever a peak is not 0
 *            by a factor of 0; in an all-zero record peak = 0 and nothing hits.
 *   Why two tests: the first finds what stands above the noise; but a strong transmitter's window side lobes and clipping products
 *            stand above the noise too, across hundreds of kHz, and the middle of that span is not the signal's frequency.  The
 *            second keeps the bins within 1 / rel of the record's strongest (rel = 16: within 12 dB).  Its price: a weak burst in
 *            the same RECORD as a much stronger one (more than rel times stronger in peak power) is not seen.  Shorter records
 *            (frames_per_record) narrow that blind spot in time; a larger rel narrows it in level.
 *   Outputs per (row, record): one tfrec_amd_occupancy and N / 32 bitmap words: bit (k & 31) of word (k >> 5) is hit[k].  n_hit is
 *            the number of set bits, n_frames the record's.  top is not stored: 16 bytes keep the struct a power of two, and a caller
 *            who wants it has peak[] from tfrec_amd_read_spectrum.
 *   Nothing is carried between submits.  Grouping the hits of a whole recording into channels is host work: tfrec_gpu -A and
 *            tfrec_amd/occupancy.py: channels() do it; DESIGN.md 6l states the rule.
 *   Defaults: the library has none.  tfrec_gpu and the Python binding use ratio = 32 (a windowed noise bin's power is close to
 *            exponentially distributed: P(p > 32 mean) = e^-32 per frame and bin) and rel = 16 (chosen on one synthetic recording);
 *            neither is a measurement of real recordings.
 * tfrec_amd_enable_occupancy: allowed only after tfrec_amd_enable_spectrum and before the first submit.  Per FIFO set
 * (TFREC_AMD_FIFO_DEPTH of them) it allocates max_rows * max_records * (16 + N / 8) bytes of device memory, max_rows, max_records
 * and N the spectrum's; tfrec_amd_get_memory counts it.  Its one kernel runs on the spectrum's stream, directly behind the
 * spectrum's kernel: no stream or event of its own.
 * Errors: a NULL context, ratio or rel outside its range, a context without the spectrum, or a second call: TFREC_AMD_E_INVAL;
 * after the first submit: TFREC_AMD_E_STATE, as for a poisoned context; TFREC_AMD_E_NOMEM leaves the context exactly as it was before
 * the call, the spectrum included.  A context on which it was never called launches what it launched before. */
typedef struct {            /* 16 bytes */
	uint64_t floor;         /* the lower median of m */
	uint32_t n_hit;         /* bins hit */
	uint32_t n_frames;      /* the record's frames (tfrec_amd_read_spectrum's n_frames) */
} tfrec_amd_occupancy;
int tfrec_amd_enable_occupancy(tfrec_amd_ctx *ctx, uint32_t ratio, uint32_t rel);
/* The occupancy records of one input row of the OLDEST undrained submit, with the conventions of tfrec_amd_read_spectrum (waits for
 * the submit; call it BEFORE tfrec_amd_drain_events pops it; reading pops nothing): recs[r], bitmap[r * (N / 32) + w] for r <
 * *n_records; cap_records is the room in records.  recs and bitmap may be NULL with cap_records 0 to fetch only *n_records.
 * Errors: the detector not enabled, a row the submit's spectrum does not cover, n_records NULL: TFREC_AMD_E_INVAL; the room too
 * small (or a NULL array with records to deliver): TFREC_AMD_E_INVAL, nothing is written, but *n_records is set; nothing undrained
 * or a poisoned context: TFREC_AMD_E_STATE. */
int tfrec_amd_read_occupancy(tfrec_amd_ctx *ctx, int32_t row, tfrec_amd_occupancy *recs, uint32_t *bitmap, size_t cap_records,
			     int *n_records);

/* The dB value the reference demodulator passes to decoder::flush for this slot, computed with the
 * reference's host expressions (tfa1.cpp:180, tfa2.cpp:434, whb.cpp:696) including (int)(10*log10(0)). */
int tfrec_amd_rssi_db(int slot, int64_t rssi_raw);

/* Parity/debug (TFREC_AMD_F_INPUT_10X or tfrec_amd_create_rate): the 1.536 MS/s int16 IQ the 10:1 or the resampling stage produced
 * for the last submit. */
int tfrec_amd_read_stage0(tfrec_amd_ctx *ctx, int stream, int16_t *out, size_t n_pairs);
/* Parity/debug: copy the decimated int16 IQ of the last submit for one stream (n_pairs*2 int16). */
int tfrec_amd_read_decimated(tfrec_amd_ctx *ctx, int stream, int16_t *out, size_t n_pairs);
/* fm_dev (dsp_stuff.cpp:284-292) is (int)(atan2(cj, cr) * 16384/pi) in double.  The device evaluates its own atan2
 * (4e-12 in the scaled angle); every sample whose scaled angle lies within 1e-9 of an integer is decided by an exact
 * slow path (double-double; the result the reference computes under a correctly rounded atan2), and the decisions are
 * logged (the first 62 per submit) and checked against THIS host's libm -- the arithmetic the reference binary uses
 * here -- when the submit is drained.  A run certifies itself: host_mismatch == 0 means every logged decision equals
 * the reference's; `undecidable` counts samples so close to a rounding midpoint of atan2 (< 0.06 ulp) that glibc's
 * documented error (0.55 ulp) lets the reference itself round either way (expected ~2e-13 per sample). */
typedef struct {
	uint64_t resolved;      /* samples decided by the slow path (of the submits drained so far) */
	uint64_t host_verified; /* ... of which were logged and compared with the host's libm */
	uint64_t host_mismatch; /* ... and differed from it */
	uint64_t undecidable;   /* slow-path samples within 0.06 ulp of an atan2 rounding midpoint */
	uint64_t reserved[4];
} tfrec_amd_fm_stats;
int tfrec_amd_get_fm_stats(tfrec_amd_ctx *ctx, tfrec_amd_fm_stats *out);
/* Samples decided by the slow path, including submits not drained yet (waits for them). */
int tfrec_amd_atan_uncertain(tfrec_amd_ctx *ctx, uint64_t *n);
/* Parity probe: the device's fm_dev on n 16-byte records -- kind 0: int32 quadruples (ar, aj, br, bj) = the arguments
 * of dsp_stuff.cpp:284; kind 1: int64 pairs (cr, cj) = its cross terms (:288-289), for directions no int16 quadruple
 * reaches; kind 2: the device's fm_dev_nrzs (dsp_stuff.cpp:269-279, with its +-1e9 clamp) on int32 quadruples.
 * out[n].  No context needed.  stats (may be NULL): as above, for this call. */
int tfrec_amd_fm_dev_probe(int device, int kind, const void *records, size_t n, int32_t *out, tfrec_amd_fm_stats *stats);
/* Parity probe: the device's iir2 (dsp_stuff.cpp:28-56: set(cutoff), then step() over in[0 .. n) from the zero state) ->
 * out[n], the outputs as doubles, bit for bit what the reference's normative build produces.  form 0:
 * the step as the reference associates it; form 1: the 3-multiply form the biquad passes and WHB stage 2 run (csrc/dsp_dev.h:
 * iir_step_t).  cutoff: iir2's argument, e.g. 0.5 / spb (tfa2.cpp:321), 2.0 / 64, 0.0025 / 64 (whb.cpp:610-611).  No context. */
int tfrec_amd_iir_probe(int device, double cutoff, int form, const double *in, size_t n, double *out);
/* Parity probe, like tfrec_amd_iir_probe: the output row of the fp64 biquad of (slot, stream) -- slot 1-3 the TFA_2 family
 * (tfa2.cpp:362, the int16 values widened), slot 4 WHB stage 1 (whb.cpp:651-652) -- as the biquad passes (csrc/biquad.h) left it
 * for the most recently drained submit, read from the table set that submit used, after a sync.  The row is window-relative:
 * window j of the chain in that submit, opened at decimated sample og, owns the 32-sample slots (og >> 5) + j ..., and its slot i
 * holds the outputs of samples og + 32 i ...; values outside the windows are unspecified.  *n_slots: the slots of a row; out
 * takes 32 values per slot (cap_values >= 32 * *n_slots), or out = NULL with cap_values = 0 to ask for *n_slots alone.
 * TFREC_AMD_E_INVAL, with nothing written: slot 0 (TFA_1 has no biquad), a slot outside the context's types, a context with
 * TFREC_AMD_F_SERIAL_CHAINS (it keeps no such rows), no submit drained yet, cap_values too small. */
int tfrec_amd_read_biquad_row(tfrec_amd_ctx *ctx, int slot, int stream, int32_t *out, size_t cap_values, uint32_t *n_slots);
int tfrec_amd_get_timings(tfrec_amd_ctx *ctx, tfrec_amd_timings *out);
/* Cumulative counters of the speculative stages (window-parallel pipeline only).  They only describe how the work
 * was done -- results do not depend on them. */
typedef struct {
	uint64_t biquad_segments;    /* biquad segments processed */
	uint64_t biquad_unconverged; /* parallel repair runs that reached the end of their segment without joining the
				        speculative trajectory (normal for a chain's short last segment) */
	uint64_t biquad_serial;      /* segments the chain walk had to repair serially */
	uint64_t tfa2_resliced;      /* tfa2 windows sliced again because the last_bit_idx assumption did not hold */
	uint64_t tfa1_recomputed;    /* 64-sample steps of long TFA_1 windows whose pre-computed peak detector piece did not
				        start from the true value and were recomputed */
	uint64_t biquad_repair_slots; /* 32-sample slots the first repair pass ran (a segment has up to kSegSlots of them, csrc/tfrec_dev.h: 256 in the product build) */
	uint64_t whb_respeculated;   /* (stream, submit) pairs whose lane-parallel WHB decision levels did not reproduce the exact
				        recurrence's decisions and were demodulated again by the exact kernel */
	uint64_t tfa1_scalar_groups; /* groups of 64 steps (4096 samples) of long TFA_1 windows that the lane-per-step cooperative slicer
				        left to its scalar walk (entered without a last_bit_idx and a candidate at a block's second
				        sample, a stale peak-detector piece, > 64 bits in a lane) */
	uint64_t tfa2_scalar_groups; /* ... of the TFA_2 family (more than 16 rounds of re-walking, entered with a block-relative 0) */
	uint64_t tfa1_vector_groups; /* groups the lane-per-step form did (counted by the experiments build of the library only, csrc/knobs.h;
				        0 otherwise: nearly every wave of the slicers would add to them): TFA_1, */
	uint64_t tfa2_vector_groups; /* TFA_2 family */
} tfrec_amd_stats;
int tfrec_amd_get_stats(tfrec_amd_ctx *ctx, tfrec_amd_stats *out);
/* Layout of the context's pipeline, named by its number of CHAIN streams: 6 = deep (default: the filter stage of submit
 * k+1 runs beside the slicer/decoder stage of submit k; plus the front-end stream and two low-priority streams for the
 * discriminator pass and the drain's copy), 4 = shallow (environment TFREC_AMD_DEEP=0 when the context is
 * created), 2 = the serial cross-check (TFREC_AMD_F_SERIAL_CHAINS).  Results do not depend on it.  No reference
 * counterpart. */
int tfrec_amd_get_layout(tfrec_amd_ctx *ctx, int *n_streams);
/* Device memory the context holds (front-end outputs, window tables, biquad outputs, state, event buffers: one set per
 * submit that may be in flight) and the page-locked host memory of its drain buffers, in bytes.  The caller's input
 * batches are not counted.  No reference counterpart. */
int tfrec_amd_get_memory(tfrec_amd_ctx *ctx, uint64_t *device_bytes, uint64_t *pinned_host_bytes);
/* Current trigger threshold of one stream (auto mode, fm_demod.cpp:58-73, moves it; a fixed stream returns its own thresh).
 * Per stream: the settings the last submit ran with (tfrec_amd_configure_streams takes effect with the next submit). */
int tfrec_amd_read_thresh(tfrec_amd_ctx *ctx, int stream, int *thresh);

#ifdef __cplusplus
}
#endif
#endif
