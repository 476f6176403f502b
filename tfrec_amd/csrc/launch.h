// tfrec_amd/csrc/launch.h -- the host-side launchers: the only interface between frontend.hip, chains.hip, chains2.hip (which define
// them beside their kernels) and capi.hip (which calls them), declared here once and included by all four behind tfrec_dev.h.
// The records are host-side aggregates, filled with designated initialisers where a submit is made (capi_submit.h) and unpacked
// into the kernels' arguments inside the launchers: none of them is a kernel argument.
#pragma once

namespace tfrec {

// A submit's front-end output (capi_submit.h: front_out): what the front end writes and every later stage works on
struct FrontOut {
	uint32_t *dec;             size_t dec_stride;    // [n_streams][dec_stride] decimated pairs
	unsigned long long *mask;  size_t mask_stride;   // [n_streams][mask_stride] trigger mask
	uint32_t *prevdec;                               // [n_streams] the decimated sample before the submit's first one
	int16_t *fmdev;            size_t fmdev_stride;  // [n_streams][fmdev_stride] the discriminator's output
	int n_streams, n_blocks;
};
// A carried history of the input, flipped per submit: `in` is read, `out` written for the next submit
struct History {
	const uint8_t *in;
	uint8_t *out;
};
// A rate's tap table on the device: [q][t] floats, h / 1024 -- or, rs_streamed(q, t), resample_stream_kernel's (formats.h)
struct RateTable {
	int p, q, t;
	const float *taps;
};
// The recorder's carried state, the one working set of its kernels, and the set's totals, table and pool
struct CaptureBufs {
	CaptureState *state;
	CaptureStage *stage;
	int stage_cap;
	uint2 *cnt;
	uint4 *base;
	CaptureHeader *hdr;
	tfrec_amd_run *runs;
	uint32_t *pool;
	uint32_t max_runs;
	unsigned long long max_samples;
};
// The burst track's buffers (track.h): the set's records, bitmap and centre indices, the carried 16 pairs and chain position of every
// stream, and L; in auto-centre mode (centre.h) also the set's centre records, every stream's carried index and centre, and K; in
// phase mode (phase.h) those too, carry holds 80 pairs per stream, and m
struct TrackBufs {
	tfrec_amd_track *recs;
	uint32_t *words;
	const int32_t *centre;
	uint32_t *carry, *prior;
	int smooth;
	tfrec_amd_track_centre *cen;
	int2 *ccarry;
	int head;
	int lag;
};
// The burst sync's buffers and settings (sync.h): the set's records and match bitmap, the set's track bitmap, the carried 64 words
// of track bits and H of every stream
struct SyncBufs {
	tfrec_amd_burst_sync *recs;
	uint32_t *words;
	const uint32_t *track;
	uint32_t *carry, *hist;
	int rate, n_bits, max_errors;
	uint32_t flags;
	unsigned long long pattern;
};
// The line code's buffers and settings (linecode.h): the set's records and coded bitmap, the set's track records and bitmap, the
// carried 64 words of track bits and H of every stream
struct CodeBufs {
	tfrec_amd_track *recs;
	uint32_t *words;
	const tfrec_amd_track *trecs;
	const uint32_t *track;
	uint32_t *carry, *hist;
	int rate;
	uint32_t taps, flags;
};
// The frame check's buffers and settings (crc.h): the set's records and check bitmap, the input bitmap of the same set (the coded
// one where the line code is on, else the track's), the carried 512 words of input bits and H of every stream, the term table
// (crc_table.h: n_terms pairs (off, col)), D, r0 and the CRC's width
struct CrcBufs {
	tfrec_amd_burst_crc *recs;
	uint32_t *words;
	const uint32_t *track;
	uint32_t *carry, *hist;
	const uint2 *terms;
	int n_terms, reach, width;
	uint32_t r0;
};
// The spectrum of rows 0 .. n_rows - 1 of a submit of n_in complex samples per row, and the set's records: [rows][max_records][n_bins]
// sums and peaks, [rows][max_records] frame counts.  launch_occupancy reads what launch_spectrum has just queued on the stream.
struct SpectrumBufs {
	int n_rows;
	long n_in;
	int n_bins, g;
	size_t max_records;
	unsigned long long *sum, *peak;
	uint32_t *nfr;
};
// A sparse submit's tables (tfrec_amd_submit_runs): { start, end, pool offset low, high } per run, the pool, the pair ahead of every
// run, first_run[n_streams + 1] and the prevdec overrides ({ use, pair } per stream)
struct RunsTables {
	const uint4 *tab;
	const uint32_t *pool, *pre;
	const int32_t *first;
	const uint2 *ov;
};

// ---- frontend.hip: the pre-stages (chan != nullptr: per stream {inc, phase, input row, 0}) ...
hipError_t launch_decim10(hipStream_t st, const uint8_t *iq, size_t stride, int n_streams, int n_blocks, History hist, uint32_t *out,
			  size_t out_stride, const uint4 *chan);
hipError_t launch_resample(hipStream_t st, int fmt, const uint8_t *iq, size_t stride, int n_streams, int n_blocks, const RateTable &rate,
			   History hist, uint32_t *out, size_t out_stride, const uint4 *chan, bool tuned);
hipError_t launch_ingest(hipStream_t st, int fmt, const uint8_t *iq, size_t stride, int n_streams, int n_blocks, uint32_t *out,
			 size_t out_stride, const uint4 *chan);
hipError_t launch_correct(hipStream_t st, int fmt, const uint8_t *iq, size_t stride, int n_rows, long n_in, const CorrectBufs &b);
// ... the front ends (scfg != nullptr: every stream's own threshold) ...
hipError_t launch_frontend(hipStream_t st, const uint8_t *iq, size_t stride, History tail, const FrontOut &o, int thresh,
			   const FrontTapsCfg &taps, bool in16, const uint2 *tune, const uint4 *chan);
hipError_t launch_decin(hipStream_t st, const uint8_t *in, size_t stride, const uint4 *chan, const FrontOut &o, uint32_t *last, int thresh,
			const StreamCfg *scfg);
hipError_t launch_decin_runs(hipStream_t st, const RunsTables &r, const FrontOut &o, uint32_t *last, int thresh, const StreamCfg *scfg);
hipError_t launch_fmdev(hipStream_t st, const FrontOut &o, EventBuf *eb, int wmax, double flag_eps);
// ... the side outputs ...
hipError_t launch_levels(hipStream_t st, const FrontOut &o, LevelState *lev, const StreamCfg *scfg, tfrec_amd_level *out);
hipError_t launch_capture(hipStream_t st, const FrontOut &o, long long sample_base, const CaptureBufs &b, const StreamCfg *scfg);
hipError_t launch_capture_pre(hipStream_t st, const FrontOut &o, long long sample_base, const CaptureBufs &b, uint32_t *pre);
hipError_t launch_burst_meter(hipStream_t st, const FrontOut &o, const CaptureBufs &b, tfrec_amd_burst *out);
hipError_t launch_burst_envelope(hipStream_t st, const FrontOut &o, const CaptureBufs &b, tfrec_amd_envelope *out);
hipError_t launch_burst_clock(hipStream_t st, const FrontOut &o, const CaptureBufs &b, tfrec_amd_clock *out);
hipError_t launch_burst_track(hipStream_t st, const FrontOut &o, const CaptureBufs &b, const TrackBufs &k);
hipError_t launch_burst_track_amplitude(hipStream_t st, const FrontOut &o, const CaptureBufs &b, const TrackBufs &k);  // (k.centre: the levels)
hipError_t launch_burst_track_auto(hipStream_t st, const FrontOut &o, const CaptureBufs &b, const TrackBufs &k);  // (k.centre: the set centres in Hz)
hipError_t launch_burst_track_phase(hipStream_t st, const FrontOut &o, const CaptureBufs &b, const TrackBufs &k);  // (k.centre: the set centres in Hz; k.carry: 80 pairs a stream)
hipError_t launch_burst_sync(hipStream_t st, const FrontOut &o, const CaptureBufs &b, const SyncBufs &k);
hipError_t launch_burst_code(hipStream_t st, const FrontOut &o, const CaptureBufs &b, const CodeBufs &k);
hipError_t launch_burst_crc(hipStream_t st, const FrontOut &o, const CaptureBufs &b, const CrcBufs &k);
hipError_t launch_spectrum(hipStream_t st, int fmt, const uint8_t *iq, size_t stride, const SpectrumBufs &b);
hipError_t launch_occupancy(hipStream_t st, const SpectrumBufs &b, uint32_t ratio, uint32_t rel, tfrec_amd_occupancy *recs, uint32_t *bits);
// ... and the parity probes
hipError_t launch_fm_probe(hipStream_t st, const int32_t *quads, size_t n, int32_t *out, EventBuf *eb, int kind);
hipError_t launch_iir_probe(hipStream_t st, const double *in, size_t n, const BiquadCoef &c, double *out, int form);
// ---- chains.hip: the serial chains
hipError_t launch_chains(hipStream_t st, const FrontOut &o, long long sample_base, const ChainLaunch &L, tfrec_amd_event *events,
			 EventBuf *eb, uint32_t flags);
// ---- chains2.hip: the auto threshold and the window-parallel pipeline
hipError_t launch_threshold(hipStream_t st, const FrontOut &o, FskState *fsk, int wmax, const StreamCfg *scfg);
hipError_t launch_pipeline(const PipeCtl &P, const FrontOut &o, long long sample_base, const ChainLaunch &L, const WinTables &T, int16_t *ld16,
			   int32_t *dev32, tfrec_amd_event *events, EventBuf *eb, uint32_t flags);
hipError_t whb_chain_lds_optin();
// ---- capi.hip (state.h): a save's gather of the listed streams' carried state into the staging buffer, or a load's scatter
struct StateTable;
hipError_t launch_stream_state(hipStream_t st, bool load, const StateTable &T, const int32_t *list, int n_list, uint8_t *stage);

}  // namespace tfrec
