// tfrec_amd/host/gpu_engine.h -- batched counterpart of the reference's engine (engine.h:21-45, engine.cpp:46-94).
//
// engine::run reads one dump file block by block and pushes every block through process_iq + fsk_demod::process.
// gpu_engine::run does the same for N dump files at once, on one or several GPUs: blocks are staged to the devices
// through the C ABI (include/tfrec_amd.h) and the decoder flush events that come back are replayed, per stream and
// in time order, into ordinary decoder objects through decoder::store_bytes + decoder::flush -- the reference's own
// test entry (main.cpp:45-49).
//
// The decoder classes are the reference's: built with -DTFREC_AMD_REFERENCE_PLUGINS -I<baycom/tfrec> this file includes
// the reference's own decoder.h / tfa1.h / tfa2.h / whb.h and the adapter links against the reference's own objects
// (INTEGRATION.md section 3); otherwise it uses the mirror in plugin.h (same declarations; the reference's sources do
// not travel to the GPU box).  Nothing here touches a decoder beyond its public reference interface.
#ifndef TFREC_AMD_HOST_GPU_ENGINE_H
#define TFREC_AMD_HOST_GPU_ENGINE_H

#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "job.h"
#ifdef TFREC_AMD_REFERENCE_PLUGINS
#include "decoder.h"
#include "tfa1.h"
#include "tfa2.h"
#include "whb.h"
#else
#include "plugin.h"
#endif

// Batched result sink.  The reference runs system("<handler> <args>") once per telegram
// (decoder.cpp:67-96): one fork+exec per record does not scale to thousands of streams.  With a sink the SAME argument
// string (id temp hum seq alarm rssi flags ts) goes to it instead, tagged with the stream; the engine flushes the sink
// once per batch.
class batch_sink {
public:
	virtual ~batch_sink() {}
	virtual void put(int stream, const char *args) = 0;
};

// the handler's argument list of decoder.cpp:67-96 (without the command), for a decoder of type dec_type
void tfrec_handler_args(const sensordata_t &d, sensor_e dec_type, char *out, size_t n);

// A protocol handler of the reference (Base = tfa1_decoder, tfa2_decoder, whb_decoder: unchanged) whose
// execute_handler() -- virtual in the reference, decoder.h:42 -- hands the record to the engine's sink when there is one.
template <class Base>
class sinked_decoder : public Base {
public:
	sinked_decoder(sensor_e t, batch_sink *const *sink_, int stream_) : Base(t), sink(sink_), stream(stream_) {}
	void execute_handler(sensordata_t &d)
	{
		if (*sink) {
			char args[384];
			tfrec_handler_args(d, this->get_type(), args, sizeof(args));
			(*sink)->put(stream, args);
		} else {
			Base::execute_handler(d);
		}
	}

private:
	batch_sink *const *sink;
	int stream;
};

// One long-lived handler process for ALL streams: records go to its stdin, one line each,
// "<stream> <id> <temp> <hum> <seq> <alarm> <rssi> <flags> <ts>" -- the reference's handler arguments
// prefixed with the stream index -- written once per batch.
class pipe_sink : public batch_sink {
public:
	explicit pipe_sink(const char *command);
	~pipe_sink();
	void put(int stream, const char *args);
	void flush();
	long records() const { return n_records; }

private:
	FILE *pipe;
	std::string pending;
	long n_records;
};

// The slot-indexed protocol handlers of one stream (NULL: the type is not in `types`), registered like main.cpp:173-218
std::vector<decoder *> make_decoders(int types, batch_sink *const *sink, int stream);

class gpu_engine {
public:
	// types: -T bit mask; thresh: -t; filter: -W; dbg: -1 quiet, 0 normal, >=1 debug (main.cpp:97).
	// devices: HIP device ordinals; the streams (dump files) are sharded over them by index, contiguous ranges, no
	// exchange between devices; an ordinal may appear more than once (several contexts on one GPU).
	// per_file (tfrec_gpu -p): each file's own settings, one per file, or empty: (types, thresh, filter) for every file.  A
	// device's context builds the union of its files' types and has (thresh, filter) as defaults; each file's decoders are
	// its own types', and a stream whose file's settings differ from the context's is configured
	// (tfrec_amd_configure_streams) before the file's first batch -- and tuned (tfrec_amd_tune_streams) when its tune is not 0.
	gpu_engine(const std::vector<std::string> &dumpfiles, int types, int thresh, int filter, int dbg,
		   const std::vector<int> &devices, int blocks_per_submit,
		   const std::vector<file_settings> &per_file = std::vector<file_settings>());
	~gpu_engine();
	// exec: per-telegram handler as the reference's -e (system() per record); batched: the same command started
	// once, records on its stdin (pipe_sink); mode: the reference's -m (1 = summary at the end)
	void set_handler(const char *exec, bool batched, int mode);
	// BITS-mode replay (SURVEY 8b "In BITS mode call dec->store_bit(b) per bit then flush"): the context reports every bit
	// the demodulators hand to decoder::store_bit (TFREC_AMD_F_BITS) and every flush; the decoders then run exactly as
	// inside the reference -- including what store_bit itself prints (tfa2.cpp:294-300 "Inverted SYNC").  Default off:
	// the byte-level replay (store_bytes + flush) moves 64 bytes per window instead of every bit.
	void set_bits_replay(bool on) { job.bits_replay = on; }
	// -n: at most n streams per device context.  The dump files of a device go through them as a queue, in command-line order:
	// when a file's last block has been submitted its stream is reset (tfrec_amd_reset_streams) -- or configured and / or tuned
	// for the next file, when that one's settings or tune differ -- and the next file starts there with the next batch.  0 (default): one stream
	// per file for the whole job.  A batch that carries a reset does not overlap the batch before it on the GPU (DESIGN.md
	// 6b): a queue of mixed-length files runs at about half the throughput.
	void set_slots(int n) { job.slots = n; }
	// -x: the dump files are 15.36 MS/s u8 dumps (TFREC_AMD_F_INPUT_10X, blocks of TFREC_AMD_BLOCK_BYTES_10X), and a file's tune
	// is a wide tune (tfrec_amd_tune_streams_wide, up to +-7679 kHz) ahead of the 10:1 stage.
	// In both modes, without -n: a path given to several -L is opened and read once and occupies one input row of the batch; its
	// streams are mapped to it (tfrec_amd_map_streams).  Decoders, stream indices and output order stay per -L occurrence.
	void set_wide(bool on) { job.wide = on; }
	// -r: the dump files are u8 dumps at 1536000 p / q samples per second (tfrec_amd_create_rate).  A submit then
	// carries a multiple of `unit` blocks, q / gcd(q, 64) (the caller rounds blocks_per_submit up to one), a file is read in
	// pieces of that many blocks and its trailing partial piece is dropped; everything else -- the tail of a file, -n, -d,
	// shared paths, tunes and settings -- is as without it, and a file's tune beyond +-767 kHz (up to half the rate) becomes the
	// input-rate tune ahead of the resampler (tfrec_amd_tune_streams_input).  Excludes set_wide.
	void set_rate(int p, int q) { job.rate_p = p; job.rate_q = q; }
	// -F: the dump files hold TFREC_AMD_FMT_* samples instead of u8 (tfrec_amd_create_format), at the rate of
	// set_rate or -- without one -- at 1.536 MS/s.  A block of a file is 65536 p / q * bytes per complex sample / 2 bytes, and a
	// shorter file is padded with the format's silence (zero); everything else is as with u8.  Excludes set_wide.
	void set_format(int format) { job.fmt = format; }
	// -s: scan mode.  The dump files are ONE recording given once per channel, khz[i] the receive frequency of
	// file i (ascending; the files' tunes place them): the streams share the recording's input row as repeated paths always do,
	// the context runs with TFREC_AMD_F_LEVELS, and instead of replaying telegrams into the decoders run() sums every channel's
	// level records (tfrec_amd_read_levels, the blocks the file really holds) and counts its events with status 1.  It prints
	// the channel list to stderr before a device is opened and the table to stdout at the end: per channel
	//   scan <kHz> blocks=<n> mean_pwr=<sum pwr_sum / (8192 n)> peak=<max pwr_max> over=<sum n_over> triggered=<sum triggered>
	//        thresh=<the last block's> telegrams=<events with status 1>
	// preceded, with dbg > 0, by the reference's per-block line "<kHz> Trigger ratio <triggered>/8192, avg <triggered_avg>"
	// (fm_demod.cpp:61) for every block.  One device, no -n.
	void set_scan(const std::vector<long> &khz) { job.scan = true; job.scan_khz = khz; }
	// -S: the squelched recorder (tfrec_amd_enable_capture).  Every context captures the IQ of its streams' trigger
	// windows; run() writes <prefix>.idx -- text, one line "<file index> <stream> <start_sample> <n_samples> <thresh> <flags>" per run
	// in submit order, stream = the file's stream on its device, start_sample counted within the file -- and, for every file with
	// a run, <prefix>.<file index>.cs16: the file's captured samples appended submit by submit, 384 kS/s int16 interleaved I, Q.
	// <prefix>.<file index>.pre holds one int16 (I, Q) per .idx line of the file, in .idx order: the decimated sample just ahead of
	// the run (tfrec_amd_enable_capture_pre) -- with it set_replay reproduces the recording's events.
	// The capture is sized from the batch's blocks and the stream count so that no submit can overflow it; should one, a warning
	// goes to stderr per submit and the run goes on.  Runs are cut at the file's end (the padding behind it is not the file's).
	void set_capture(const std::string &prefix) { job.capture = true; job.cap_prefix = prefix; }
	// -P: the power spectrum of the one -L file's input row (tfrec_amd_enable_spectrum on row 0): n_bins bins,
	// frames_per_record frames per record, the file recorded at center_khz.  run() lists the bins' frequencies on stderr before a
	// device is opened ("spec bin <kHz>", ascending) and prints, behind the telegram output and in ascending frequency, per bin
	//   spec <kHz, 3 decimals> mean=<total sum / total frames> peak=<max over the records>
	// preceded, with dbg > 0, by "spec-rec <record> <kHz> sum=<..> peak=<..> frames=<..>" per record (counted through the file) and bin.
	// The bin's frequency is center + (k < N/2 ? k : k - N) fs_in / N.  One file, one device, no -n.
	void set_spectrum(int n_bins, int frames_per_record, long center_khz)
	{
		job.spectrum = true;
		job.spec_n = n_bins;
		job.spec_g = frames_per_record;
		job.spec_center = center_khz;
	}
	// -A, pass 1: with set_spectrum, the occupancy detector on the file's spectrum records
	// (tfrec_amd_enable_occupancy: ratio, rel).  run() reads the detector's records instead of the spectrum's, replays no telegram
	// and prints no spectrum table: it counts, per bin, the records of the file in which the bin was hit (a record that begins
	// behind the file's end, in the padding of its last batch, is not counted), groups them (occupancy_channels, join_hz) and
	// prints, in ascending frequency,
	//   found <kHz> bins=<lo>..<hi> hits=<max in group>/<records>[ out-of-range]
	//   carrier <kHz> hits=<h>/<records>
	// preceded, with dbg > 0, by "occ-rec <record> floor=<..> hits=<n_hit> frames=<..>" per record.  found_khz() then lists the
	// channels a scan can reach, ascending.
	void set_occupancy(int ratio, int rel, long join_hz)
	{
		job.occ_ratio = ratio;
		job.occ_rel = rel;
		job.occ_join = join_hz;
	}
	const std::vector<long> &found_khz() const { return occ_found; }
	// -z: the DC blocker (tfrec_amd_create_dc) over `windows` windows of 512 input samples, on every input row of every
	// context: a file's row (a path shared by several streams: its one row) is corrected once, ahead of every tune.  With -n the
	// row of a stream that starts a new file has its DC state reset with the stream (tfrec_amd_reset_dc_rows).  With dbg > 0 run()
	// prints "dc <file> I=<d> Q=<d>" per submit and file: the estimate of the submit's last window of the file's row.  Under -A
	// only pass 2 is given it: pass 1's spectrum reads the raw rows either way.  Excludes set_wide.
	void set_dc(int windows) { job.dc_windows = windows; }
	// -Z: the IQ balancer (tfrec_amd_create_iq) over `windows` of the same windows, behind the DC blocker of set_dc or
	// without one, on every input row of every context, sized and reset as the blocker is.  With dbg > 0 run() prints
	// "iq <file> t=<t> g=<g>" per submit and file: the estimate of the submit's last window of the file's row.  Excludes set_wide.
	void set_iq(int windows) { job.iq_windows = windows; }
	// -R: replay a capture.  The engine's files are the capture's -- captures[i] is file i of the job, read back whole,
	// and a file's length is its last run's end rounded up to blocks --; every context takes channel-rate input
	// (tfrec_amd_create_decimated) and is fed sparse submits (tfrec_amd_submit_runs) cut by the batch plan, so -b, -n and -d work as
	// with dumps.  captures outlives the engine.  Excludes every set_* that concerns the input.
	void set_replay(const std::vector<replay_file> &captures) { job.replay = &captures; }
	// -M: the burst meter (tfrec_amd_enable_burst_meter).  Every context enables the recorder -- set_capture's, or with
	// set_capture's room for runs and a pool of one pair -- and the meter on it; run() merges the records' chains across the batches
	// of a file (job.h: chain_merger; a chain still open at the file's end is flushed there) and prints, as each burst ends,
	//   burst <file> <start_sample> <n_samples> <pwr_max> <centre_hz|-> <deviation_hz|->
	// (job.h: burst_summary; "-": no bin is occupied).  With set_scan the lines are not printed: the table's lines end in
	// " burst_centre=<Hz|->", the centre of the channel's burst with the largest pwr_max.  Under -A it is the scan's, not pass 1's.
	// Neither the 1/16 rule behind the summary nor its usefulness has been measured on real recordings.
	void set_meter() { job.meter = true; }
	// -Q: the burst envelope (tfrec_amd_enable_burst_envelope), with or without -M.  Every context enables the recorder
	// as for -M and the envelope on it; run() merges the records' chains across the batches of a file (job.h: chain_merger; a
	// chain still open at the file's end is flushed there, OPEN) and prints, as each burst ends,
	//   extent <file> <start_sample> <n_samples> <burst_samples> <n_over> <n_gaps> <max_gap> <ratio_c|-> <snr_db|->
	// (job.h: envelope_summary; ratio_c in hundredths as %d.%02d, "-": undefined).  With set_scan the lines are not printed: the
	// table's lines end in " burst_snr=<ratio_c|->", the median ratio_c of the channel's bursts that have one (of an even count the
	// lower middle one).  Under -A it is the scan's, not pass 1's.
	void set_envelope() { job.envelope = true; }
	// -C: the burst clock (tfrec_amd_enable_burst_clock), with or without -M and -Q.  Every context enables the
	// recorder as for -M and the clock on it; run() merges the records' chains across the batches of a file (job.h: chain_merger; a
	// chain still open at the file's end is flushed there, OPEN) and prints, as each burst ends,
	//   clock <file> <start_sample> <n_samples> <n_segments> <clock_hz|-> <quality|->
	// (job.h: clock_summary; quality_c in hundredths as %d.%02d, "-": no whole segment, or an empty band).  With set_scan the lines
	// are not printed: the table's lines end in " burst_clock=<Hz|->", the clock_hz of the channel's chain with the largest quality_c,
	// the earliest among equals.  Under -A it is the scan's, not pass 1's.  Neither the band, the segment length nor the usefulness
	// of quality_c has been measured on real recordings.
	void set_clock() { job.clock = true; }
	// -G: the burst track (tfrec_amd_enable_burst_track), with or without -M, -Q and -C.  Every context enables the
	// recorder with a pool for every sample (the bitmap has the pool's size) and the track on it, L = half a symbol of `rate` held
	// within 1 .. 16, every stream about centre_hz; run() merges the records' chains and their bits across the batches of a file
	// (job.h: chain_merger; a chain still open at the file's end is flushed there, OPEN; at most the first 2^20 samples of a chain
	// are kept) and prints, as each burst ends,
	//   bits <file> <start_sample> <n_samples> <burst_samples> <n_bits>[+] <hex|->
	// (job.h: track_slice, track_line: the run-length slice at `rate` of the first burst_samples = last_over + 1 samples, MSB-first;
	// "+": the chain is longer than what is kept; "-": no symbol).  Nothing of it has been measured on real recordings.
	void set_track(long rate, long centre_hz)
	{
		job.track_rate = rate;
		job.track_centre = centre_hz;
	}
	// -O (with -G): the track is the amplitude's (tfrec_amd_enable_burst_track_amplitude), L as -G's, every stream at
	// `level` (0 .. 65535, the trigger's unit); the centre is not used.  Behind each burst's bits line run() prints its pulses
	// (job.h: track_pulses, pulses_line)
	void set_track_level(long level) { job.track_level = level; }
	// -G rate,auto (with set_track(rate, 0)): the track is the auto-centre's (tfrec_amd_enable_burst_track_auto), L as -G's,
	// K = 1024, the fallback centre 0.  Ahead of each burst's bits line run() prints its centre (job.h: centre_take, centre_line)
	void set_track_auto() { job.track_auto = true; }
	// -G rate,psk[,lag] (with set_track(rate, 0)): the track is the phase mode's (tfrec_amd_enable_burst_track_phase), L as
	// -G's, K = 1024, m = lag (1 .. 64), the fallback centre 0.  Its centre records are read, merged and printed as -G rate,auto's
	void set_track_phase(int lag)
	{
		job.track_auto = true;
		job.track_lag = lag;
	}
	// -Y (with -G): the burst sync (tfrec_amd_enable_burst_sync) on the track, at -G's rate: the sync word is the low
	// n_bits of pattern, MSB first.  run() merges the sync records' chains and their match tracks beside the track's (job.h:
	// sync_merger) and prints, behind each burst's bits line, in the order of their samples,
	//   frame <file> <start_sample> <sync_sample> <errors> <+|-> <n_bits> <hex|->
	// (job.h: sync_frames, sync_line: per plateau of matches inside the burst the payload's first `bytes` bytes, read at symbol
	// centres from the plateau's middle, MSB-first; "-": the complemented word matched and the payload is complemented).  The
	// defaults -- no errors, 8 bytes, one polarity -- are not tuned on anything: nothing of it has been measured on real recordings.
	void set_sync(unsigned long long pattern, int n_bits, int errors, int bytes, bool both, bool lsb = false)
	{
		job.sync_pattern = pattern;
		job.sync_bits = n_bits;
		job.sync_errors = errors;
		job.sync_bytes = bytes;
		job.sync_both = both;
		job.sync_lsb = lsb;  // the frames' hex LSB-first per byte (job.h: sync_line)
	}
	// -U (with -G): the line code (tfrec_amd_enable_burst_code) on the track, at -G's rate: taps bit j - 1 is a delay of j
	// symbols, invert complements the coded bit.  run() merges the coded pieces' chains beside the track's (they are track pieces:
	// chain_merger<track_piece>) and prints, behind each burst's bits line,
	//   code <file> <start_sample> <n_samples> <burst_samples> <n_bits>[+] <hex|->
	// (job.h: code_line: the coded track through -G's slicer); -Y's frames are then found on and read from the coded track.  Nothing of
	// it has been measured on real recordings.
	void set_code(uint32_t taps, bool invert)
	{
		job.code_taps = taps;
		job.code_invert = invert;
	}
	// -V (with -G and -Y): the frame check (tfrec_amd_enable_burst_crc) on the track the sync reads, at -G's rate, on
	// -Y's bytes in -Y's byte order: width, poly, init, xorout, the skipped bytes and INVERT.  run() merges the check pieces'
	// chains beside the sync's (job.h: chain_merger<crc_piece>); every frame line ends in one more field, ok, bad or - (job.h:
	// crc_verdict), and behind a burst's frame lines comes
	//   crc <file> <start_sample> <n_samples> <n_ok> <sample|->
	// (job.h: crc_line).  Nothing of it has been measured on real recordings.
	void set_crc(int width, uint32_t poly, uint32_t init, uint32_t xorout, int skip, bool invert)
	{
		job.crc_width = width;
		job.crc_poly = poly;
		job.crc_init = init;
		job.crc_xorout = xorout;
		job.crc_skip = skip;
		job.crc_invert = invert;
	}
	// -k: keep.  A file is processed in whole pieces only and nothing is padded; before the first batch behind a
	// file's last one is submitted -- and at the end of the job -- its stream is saved (tfrec_amd_save_streams) to
	// <prefix>.<file index>.state, and at the end of a run without an error the bytes that did not fill a piece are written to
	// <prefix>.<file index>.rest (empty when none).  A file of no whole piece runs nothing: its .rest is all of it, its .state the
	// one it continued from, if any.
	// -K: continue.  <prefix>.<file index>.state is loaded into the file's stream before its first batch
	// (tfrec_amd_load_streams: the saved settings, which the file's own must equal -- run() fails otherwise --, and the saved tunes), the bytes of
	// <prefix>.<file index>.rest are read ahead of the file's own, and end_sample goes on counting from the saved sample count.
	// Both: one stream per file for the whole job (no -n), every path once.  The host decoders' own memory (the -m 1 table, the
	// "#nnn" counter) is not carried.  run() fails with TFREC_AMD_E_INVAL if a .state cannot be read.
	void set_keep(const std::string &prefix) { job.keep_prefix = prefix; }
	void set_continue(const std::string &prefix) { job.cont_prefix = prefix; }
	// returns 0 on success, a TFREC_AMD_E_* code otherwise
	int run();
	// decoders of stream s in slot order (NULL for slots not registered)
	decoder *get_decoder(size_t s, int slot) { return decs[s][slot]; }
	long telegrams() const { return n_telegrams; }

private:
	void replay(const tfrec_amd_event &ev);
	std::vector<std::string> files;
	std::vector<file_settings> settings;  // per file
	file_settings dflt;                   // the constructor's types, thresh, filter
	int bps;
	std::vector<int> devices;
	job_settings job;                     // the set_* calls' (job.h)
	std::vector<std::vector<decoder *> > decs;
	std::vector<long long> stream_samples;  // decimated samples each file really holds
	long n_telegrams;
	batch_sink *sink;  // (the decoders hold its address)
	pipe_sink *psink;
	int out_mode;
	std::vector<long> occ_found;
};

#endif
