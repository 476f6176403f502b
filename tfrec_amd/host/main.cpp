// tfrec_amd/host/main.cpp -- tfrec_gpu: the reference's file-replay CLI on the GPU path.
//
//   tfrec_gpu [-T hexmask] [-t thresh] [-W] [-f kHz] [-c kHz] [-x | -r Hz] [-F format] [-z [windows]] [-Z [windows]] [-q] [-D] [-B] [-d device[,device...]] [-b blocks]
//             [-n streams] [-e handler | -E handler] [-m mode] [-p settings] -L dump.iq [[-p settings] -L more.iq ...]
//   tfrec_gpu [receiver flags as above] [-c kHz] [-x | -r Hz] [-F format] [-D] -P bins[,frames_per_record] -L dump.iq
//   tfrec_gpu [-T hexmask] [-t thresh] [-W] [-c kHz] [-x | -r Hz] [-F format] [-D] [-d device] [-b blocks] -s step_kHz -L dump.iq
//   tfrec_gpu [-T hexmask] [-t thresh] [-W] [-c kHz] [-x | -r Hz] [-F format] [-D] [-d device] [-b blocks] [-P bins[,frames]]
//             -A [ratio[,rel[,join_kHz]]] -L dump.iq
//   tfrec_gpu [-T hexmask] [-t thresh] [-q] [-D] [-d device[,device...]] [-b blocks] [-n streams] [-e handler | -E handler] -R prefix
//   tfrec_gpu [-T hexmask] -X telegrams.txt
//
// Flags keep the reference's meaning (main.cpp:63-88, 107-164): -T sensor type bit mask (hex), -t trigger
// threshold (0 = auto, the default), -W wide filter, -f receive frequency in kHz, -q quiet, -D debug,
// -e handler executed for every message, -m 1 summary at exit,
// -L raw 8-bit IQ dump as written by "tfrec -S", -X hex telegrams for the byte-level test entry
// (main.cpp:24-53).  Several -L files are processed as one batch, one stream each.
// -B (not in the reference): BITS-mode replay -- every demodulated bit goes through the decoder's own store_bit
// (gpu_engine.h), so that stdout also carries what store_bit prints ("Inverted SYNC", tfa2.cpp:294-300).
// -E handler (not in the reference): the handler is started ONCE and receives the records of all
// streams on stdin, "<stream> <id> <temp> <hum> <seq> <alarm> <rssi> <flags> <ts>" per line, one write per batch.
// -n streams (not in the reference): at most this many streams per device; the -L files queue for them in order, and a
// stream whose file has ended is reset and takes the next file (gpu_engine.h).  <stream> of -E is then the file's index.
// -p T=<hex>,t=<n>,W=<0|1> (not in the reference; any of the three fields, in any order): -T, -t and -W of the -L files that
// follow it, up to the next -p -- what they would be to separate tfrec processes.  Fields left out, and files before any -p,
// take the global -T / -t / -W.  The files share one context per device (tfrec_amd_configure_streams).
// -f kHz keeps the reference's meaning, the receive frequency; -c kHz (not in the reference) is the frequency the dumps were
// recorded at, by default 868250 (the reference's default -f).  A dump cannot be retuned: the difference is applied as a
// digital shift of the recorded IQ (tfrec_amd_tune_streams), within +-767 kHz.  -p f=<kHz> sets it per file; one
// file given twice with two f= runs as two streams.
// -x (not in the reference): the -L files are 15.36 MS/s u8 dumps (ten times the rate: TFREC_AMD_F_INPUT_10X), and the whole
// difference f - c is a shift AHEAD of the 10:1 stage (tfrec_amd_tune_streams_wide), within +-7679 kHz: a receiver
// can sit anywhere in the wide dump.  With or without -x, and without -n: a path given to several -L is opened and read once and
// occupies one input row of the batch (tfrec_amd_map_streams); decoders, the -E stream index and the order of the output stay
// per -L occurrence.  With -n a repeated file is read once per occurrence, as before.
// -r Hz (not in the reference): the sample rate of the -L files, for dumps that were not recorded at 1.536 MS/s -- rtl_sdr's
// default 2048000, 2400000, 1920000 ... --: the rate is reduced to P / Q of 1536000 and the dumps are resampled on the GPU
// (tfrec_amd_create_rate; 1 < P/Q < 10, Q <= 64 or Q | 1536: every whole-kHz rate in between, 2000000, 2500000,
// 10000000, 12500000 ...).  -f / -c / -p f= reach the whole recording, |f - c| below half the
// rate: within +-767 kHz the shift acts behind the resampler (tfrec_amd_tune_streams), a larger one ahead of it, at the input
// rate (tfrec_amd_tune_streams_input).  A path given to several -L is read once, as without -r.  A submit must
// hold a whole number of 512-sample windows: -b is rounded up to the next multiple of Q / gcd(Q, 64).  Excludes -x.
// -F u8|s8|s16|f32 (not in the reference; also cu8, cs8, cs16, cf32): what the -L files hold -- rtl_sdr's offset-binary u8 (the
// default), hackrf_transfer's signed int8, the int16 of Airspy, SDRplay, USRP and rx_sdr, or the float32 of GNU Radio, SDR++, GQRX
// and SigMF cf32_le; little-endian, interleaved I, Q, without a header (tfrec_amd_create_format).  With -r the files
// are at that rate, without it at 1.536 MS/s.  A block of a file is 65536 * P / Q * bytes per complex sample / 2 bytes; -b, -n, -d,
// shared paths and -f / -c / -p f= are as with -r.  A format other than u8 excludes -x.
// -s step_kHz (not in the reference): scan ONE recording -- at 1.536 MS/s, or given with -x, or with -r / -F -- for where the energy
// and the telegrams are.  A receiver sits on every channel c + k * step (k any integer) that lies at least 192 kHz,
// half the band behind the 4:1 stage, inside the recording: |k * step * 1000| <= fs_in / 2 - 192000; at most 4096 of them.  All
// read the file once, through one input row, each with the tune -f would give it; the context runs the level meter
// (TFREC_AMD_F_LEVELS).  Telegram text is suppressed; stdout carries one line per channel in ascending frequency,
//   scan <kHz> blocks=<n> mean_pwr=<..> peak=<..> over=<..> triggered=<..> thresh=<..> telegrams=<..>
// and with -D, ahead of it, the reference's "Trigger ratio" line (fm_demod.cpp:61) of each of its blocks, prefixed with <kHz>;
// stderr lists the channels before a device is opened.  Not with -n, -p, -f, -e / -E, -X, several -L or several devices.
// -S prefix (the reference's letter, main.cpp:77 "Save IQ-file for later debugging"; here of the trigger windows only): record the
// decimated IQ of every sample at which a demodulator of the stream was triggered (tfrec_amd_enable_capture).
// <prefix>.idx gets one text line "<file index> <stream> <start_sample> <n_samples> <thresh> <flags>" per run, in submit order;
// <prefix>.<file index>.cs16 that file's captured samples, appended submit by submit: 384 kS/s int16 interleaved I, Q, which any
// SDR viewer opens (a file without a run gets none).  Works with -s -- a channel that triggers and decodes nothing is the case
// it is for -- and with everything else but -X.  <prefix>.<file index>.pre gets one int16 (I, Q) per .idx line of that file, in .idx
// order: the decimated sample just ahead of the run (tfrec_amd_enable_capture_pre), which a viewer does not need and -R does.
// -R prefix (not in the reference): replay a capture made by -S: decode the archived trigger windows again, without
// the recording -- with another -T, a stricter -t, other handlers.  One job per file index found in <prefix>.idx, its length the
// last run's end rounded up to blocks; the contexts take channel-rate input (tfrec_amd_create_decimated) and are fed the runs
// themselves (tfrec_amd_submit_runs), cut into submits by -b.  Takes -T, -t, -W (no effect: there is no filter stage), -d, -n, -b,
// -B, -m, -D, -q, -e / -E.  The replay gives the recording's own telegrams, bit for bit, when its demodulators are a subset of the
// recording's whose largest window is at most the recording's, and: with a fixed threshold, -t is at least the recorded one; with
// the auto threshold, the recording was auto from the stream's start and complete.  With -L, -x, -r, -F, -f, -c, -s, -A, -P, -z,
// -S, -p or -X, or when .idx is missing or inconsistent -- a line that does not parse, runs of a file that overlap or are out of
// order, a .cs16 or .pre shorter than the lines ask for --, it is a usage error: exit 2 before a device is opened.
// -M (not in the reference): the burst meter (tfrec_amd_enable_burst_meter): for every trigger window of every file,
// whether or not anything decoded in it, where its carrier sits relative to the receive frequency and how wide its FSK is -- what
// -f and -W are chosen from.  The contexts enable the recorder (-S's, or the table alone with a pool of one pair) and the meter;
// the pieces of a window that is cut by a submit boundary are merged, and stdout gets, as each window ends (a window still open at
// its file's end: there),
//   burst <file> <start_sample> <n_samples> <pwr_max> <centre_hz|-> <deviation_hz|->
// centre and deviation in Hz by the header's integer rule (a bin of 6 kHz is occupied when it holds 1/16 of the window's products; "-":
// none does, no carrier).  With -s or -A the lines are left out and every line of the channel table ends in burst_centre=<Hz|->, the
// centre of the channel's window with the largest pwr_max.  Works with -R, -S, -n, -d and every input option; not with -X.  The
// 1/16 rule was chosen on synthetic scenes; it has not been measured on real recordings.
// -Q (not in the reference): the burst envelope (tfrec_amd_enable_burst_envelope): for every trigger window of every
// file, whether or not anything decoded in it, how long the burst itself was (a window's n_samples includes the trigger's hold of W - 1
// samples of noise behind it), how far it stood above that noise, and whether it was one burst or a broken one.  The contexts enable
// the recorder as for -M and the envelope; the pieces of a window that is cut by a submit boundary are merged, and stdout gets, as
// each window ends (a window still open at its file's end: there),
//   extent <file> <start_sample> <n_samples> <burst_samples> <n_over> <n_gaps> <max_gap> <ratio_c|-> <snr_db|->
// burst_samples: up to the last sample over the threshold; n_over: the samples over it; n_gaps, max_gap: the stretches below it
// inside the burst; ratio_c: the burst's mean power over its tail's, exact, printed in hundredths ("-": the window is open at the
// input's end, or its tail is shorter than 64 samples or silent); snr_db = 10 log10 of it, one decimal.  With -s or -A the lines are
// left out and every line of the channel table ends in burst_snr=<ratio_c|->, the median of the channel's windows that have one.
// Works with -M, -R, -S, -n, -d and every input option; not with -X.
// -C (not in the reference): the burst clock (tfrec_amd_enable_burst_clock): for every trigger window of every file,
// whether or not anything decoded in it, how fast the burst is keyed -- what separates the five protocols (38400, 17240, 9600, 8842,
// 6000 bit/s) from each other and from foreign transmitters.  The contexts enable the recorder as for -M and the clock; the pieces of
// a window that is cut by a submit boundary are merged, and stdout gets, as each window ends (a window still open at its file's end:
// there),
//   clock <file> <start_sample> <n_samples> <n_segments> <clock_hz|-> <quality|->
// n_segments: the whole 1024-sample segments of the window that entered the spectrum; clock_hz: the peak of the spectrum of the
// window's frequency transitions between 4.5 and 48 kHz, in 375 Hz bins refined by its neighbours; quality: that peak over the
// band's mean, in hundredths ("-": the window holds no whole segment).  With -s or -A the lines are left out and every line of the
// channel table ends in burst_clock=<Hz|->, the clock of the channel's window with the largest quality.  Works with -M, -Q, -R, -S,
// -n, -d and every input option; not with -X, -k or -K.  No quality threshold is built in: noise reads a quality of a few units,
// a clean telegram 25 or more on synthetic scenes; none of it has been measured on real recordings.
// -G rate[,centre_hz] (not in the reference): the burst track (tfrec_amd_enable_burst_track): for every trigger window
// of every file, whether or not anything decoded in it, what the burst said when it is read at `rate` bit/s (1000 .. 96000: -C's
// reading) about centre_hz (|centre_hz| <= 192000, default 0: -M's reading).  The contexts enable the recorder with a pool for every
// sample and the track, smoothed over half a symbol (at most 16 samples); the pieces of a window that is cut by a submit boundary are
// merged, and stdout gets, as each window ends (a window still open at its file's end: there),
//   bits <file> <start_sample> <n_samples> <burst_samples> <n_bits>[+] <hex|->
// burst_samples: -Q's; the bits: the run-length slice of the track's first burst_samples samples, MSB-first, 1 above the centre, the
// last nibble zero-padded ("-": none; "+": the window is longer than the 2^20 samples that are kept).  It is a discriminator and a
// slicer, not a demodulator: no clock recovery, no matched filter; the golden TFA_1 and WHB scenes do not slice with it.  Works with
// -M, -Q, -C, -S, -R, -n, -d and every input option; not with -X, -k, -K, -s or -A.  Nothing of it has been measured on real
// recordings.
// -G rate,auto (not in the reference): the track in auto-centre mode (tfrec_amd_enable_burst_track_auto), for recordings that
// hold several transmitters, each with its own carrier offset: every burst is tracked about a centre measured on its own first
// 1024 samples (fewer than 65 of them over the threshold, or no bin with a sixteenth of the products: centre 0).  Ahead of each
// burst's bits line stdout gets
//   centre <file> <start_sample> <n_samples> <n_counted> <centre_hz> <deviation_hz|-> <m|f|i>
// m: measured, f: the fallback (no deviation), i: inherited from a piece the output does not hold.  A burst that begins within 1024
// samples of a batch's end is centred on what that batch holds of it.  Works where -G works, -Y included; not with -O.  Nothing of
// it has been measured on real recordings.
// -G rate,psk[,lag] (not in the reference): the track in phase mode (tfrec_amd_enable_burst_track_phase), for phase-keyed
// bursts, whose frequency does not move: a differential phase detector at a lag of a symbol (lag samples, 1 .. 64; default
// floor((768000 + rate) / (2 rate)), a usage error above 64) about the burst's own carrier, measured on its first 1024 samples.  1: the
// same phase as a symbol ago -- an NRZ-S transmitter's data bit.  -G rate,auto's centre line comes ahead of each bits line, its
// deviation always 0.  No descrambler and no byte order: the bits are the detector's.  Works where -G rate,auto works, -Y included;
// not with -O.  Nothing of it has been measured on real recordings.
// -O level (not in the reference; with -G rate, no centre): the track is the amplitude's (tfrec_amd_enable_burst_track_amplitude, DESIGN.md
// 6v), for on-off keyed bursts: 1 where the sum of L powers |I| + |Q| lies above L times level (0 .. 65535, -t's unit; L: -G's).  The
// bits line and -Y's frame lines are read off that track, and behind each bits line stdout gets
//   pulses <file> <start_sample> <n_samples> <burst_samples> <n_pulses>[+] <w0,g0,w1,...|->
// the widths in samples of the track's pulses and of the gaps between them ("-": no pulse; "+": more than the 64 pulses listed).
// Works where -G works.  A level slicer with the level the user gives (half of -M's pwr_max is a place to start, not a tuned
// default), not an AGC; nothing of it has been measured on real recordings.
// -Y hex[,errors[,bytes[,both]]] (not in the reference; with -G): the burst sync (tfrec_amd_enable_burst_sync): the
// sync word is the 2 .. 16 hex digits (8 .. 64 bits), MSB first; the track, read at -G's rate at symbol centres, may differ from it
// in `errors` places (default 0, below half the bits); both = 1 accepts the complemented word too (default 0).  Behind each burst's
// bits line stdout gets, for every plateau of matching samples inside the burst, in order,
//   frame <file> <start_sample> <sync_sample> <errors> <+|-> <n_bits> <hex|->
// sync_sample: the plateau's middle, where the word's last bit is read; the hex: the `bytes` bytes (1 .. 256, default 8) read at
// symbol centres behind it, MSB-first, as far as the burst reaches, complemented under "-".  No CRC is checked unless -V asks for it.  A word whose span
// at the rate exceeds 2047 samples is refused.  Works where -G works.  The defaults are not tuned on anything: nothing of it has
// been measured on real recordings.
// A fifth field, -Y hex,errors,bytes,both,1 (lsb): the frames' hex is LSB-first per byte -- every byte assembled with the first
// received bit as bit 0, a last partial byte zero-filled at the top, always two digits a byte; n_bits is unchanged.  The field is a
// flag that is given as 1 or left out; it is independent of -U.
// -U g3ruh|nrzi|nrzs|<hex taps>[,inv] (not in the reference; with -G): the line code (tfrec_amd_enable_burst_code), for
// transmitters that code their bits differentially or scramble them with a self-synchronising scrambler: the track XORed with
// itself delayed by j symbols at -G's rate for every set bit j - 1 of the taps (1 .. 8 hex digits, not 0; g3ruh = 10800, the taps 12
// and 17; nrzi = 1; nrzs = 1,inv), complemented under inv.  Behind each burst's bits line stdout gets
//   code <file> <start_sample> <n_samples> <burst_samples> <n_bits>[+] <hex|->
// the coded track through -G's slicer; -Y's frames are found on and read from the coded track.  Taps whose span at the rate exceeds
// 2047 samples are refused.  Works with what -G works with.  No CRC of its own (see -V), no Manchester decoding, no additive scrambler; nothing of it has
// been measured on real recordings.
// -V width,poly[,init[,xorout[,skip[,inv]]]] (not in the reference; with -G and -Y): the frame check (tfrec_amd_enable_burst_crc,
// DESIGN.md 6z): every frame's CRC, checked on the GPU on the track -Y reads.  The frame is -Y's bytes in -Y's byte order (its fifth
// field); width is 8, 16, 24 or 32, poly, init and xorout are hex, skip the bytes behind the sync word that the CRC does not cover,
// inv 1: every bit complemented.  The CRC is unreflected, its field the frame's last width / 8 bytes, big-endian.  Every frame line
// ends in one more field -- ok, bad, or - for a frame that is short or of polarity - --, and behind a burst's frame lines stdout gets
//   crc <file> <start_sample> <n_samples> <n_ok> <sample|->
// the samples of the burst at which a frame that checks ends, and where the sync word of the first would have ended: a frame finder
// for bursts whose sync word nobody knows.  With init 0 and xorout 0 a constant stretch checks too.  Not with -Y's both; a frame that
// reaches over 16383 samples at the rate is refused.  Nothing of it has been measured on real recordings.
// -P bins[,frames_per_record] (not in the reference): the power spectrum of ONE recording, beside its decoding: an
// exact integer DFT of bins = 64, 128, 256, 512 or 1024 bins over the raw input -- at 1.536 MS/s, or given with -x, or with -r / -F --,
// per record of frames_per_record frames (1 .. 16384; default: the frames one block's input holds, at least 1) the sum and the peak
// hold of every bin's power (tfrec_amd_enable_spectrum).  The file runs as one stream and is decoded as usual; behind the telegram
// output stdout carries one line per bin in ascending frequency,
//   spec <kHz, 3 decimals> mean=<total sum / total frames> peak=<max over the records>
// and with -D, ahead of that table, "spec-rec <record> <kHz> sum=<..> peak=<..> frames=<..>" per record and bin; bin k lies at
// c + (k < N/2 ? k : k - N) fs_in / N.  stderr lists the bins before a device is opened.  Not with -s, -n, -p, -X, several -L or
// several devices.
// -A [ratio[,rel[,join_kHz]]] (not in the reference): find the occupied channels of ONE recording, then scan exactly those (DESIGN.md
// 6l).  Pass 1 runs the file as one stream with the spectrum (256 bins unless -P bins[,frames] is given too; a record is the frames of
// one block's input, as -P's default) and the occupancy detector on the GPU (tfrec_amd_enable_occupancy: ratio 2 .. 4096, default 32;
// rel 1 .. 4096, default 16), counts per bin the records in which it was hit and groups the bins: a bin hit in more than half of the
// records is a carrier (continuous, like the RTL-SDR's DC spike), the others form a channel with their neighbours while the empty gap
// between them is at most join_kHz (0 .. 100000, default 50) wide.  stdout carries, in ascending frequency,
//   found <kHz> bins=<lo>..<hi> hits=<max in group>/<records>[ out-of-range]      (signed bins: k, or k - N from N/2 on)
//   carrier <kHz> hits=<h>/<records>
// (-D: per record "occ-rec <record> floor=<..> hits=<..> frames=<..>" ahead of them), where out-of-range marks a channel closer than
// 192 kHz to the recording's edge, which -s would not scan either.  Pass 2 is -s on the found channels: its "scan ..." lines.  No
// channel found: no scan.  Both passes run in this process, one after the other.  stderr lists the bins before a device is opened, as
// -P does.  Not with -s, -n, -p, -f, -e / -E, -X, -S, several -L or several devices.
// -z [windows] (not in the reference): remove every recording's DC offset on the GPU (tfrec_amd_create_dc) -- the few
// LSB a zero-IF front end adds to each rail, which keep |I| + |Q| above the threshold of the receiver on the centre channel.  Per
// rail the mean of the last `windows` windows of 512 input samples (1 .. 4096, default 2048) is subtracted, in exact integers, at
// the input rate and ahead of every tune; a path shared by several -L is corrected once.  Works with -r, -F, -c, -f, -p, -s, -S, -P,
// -A and -n (a slot that starts a new file starts a new estimate); the spectrum of -P and of -A's pass 1 stays that of the raw
// input.  With -D stdout carries "dc <file> I=<d> Q=<d>" per submit and file: the estimate of the submit's last window, in units
// of x (a u8 LSB is 64).  Not with -x or -X.
// -Z [windows] (not in the reference): remove every recording's IQ imbalance on the GPU (tfrec_amd_create_iq) -- the
// gain and phase error between the rails of a zero-IF front end, whose image of a burst at the mirror frequency decodes as a
// second transmitter.  One correction per recording, estimated in exact integers over the last `windows` windows of 512 input
// samples (1 .. 4096, default 2048), behind -z's subtraction and ahead of every tune.  It assumes proper signals: a DC offset is
// not one, so a recording that has one wants -z too.  Works with whatever -z works with, and not with what -z does not.  With -D
// stdout carries "iq <file> t=<t> g=<g>" per submit and file: the submit's last window's Q14 pair (balanced: t=0 g=16384).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "gpu_engine.h"

// one -p spec: the fields it sets (-1: left out, the global value)
struct spec {
	int types = -1, thresh = -1, filter = -1;
	long freq = -1;  // kHz
};

// a decimal integer within lo .. hi that is the whole string -> false if it is not one (out is then untouched)
static bool parse_long(const char *v, long lo, long hi, long &out)
{
	char *end = NULL;
	const long x = strtol(v, &end, 10);
	if (end == v || *end || x < lo || x > hi)
		return false;
	out = x;
	return true;
}

// a frequency in kHz: a decimal integer > 0 -> false if it is not one
static bool parse_khz(const char *v, long &out) { return parse_long(v, 1, 100000000L, out); }

// the optional argument of -A and -z: attached (-z64, -A32,16), or the next word where that starts with a digit; NULL: none
static const char *optional_arg(int argc, char **argv)
{
	if (!optarg && optind < argc && argv[optind][0] >= '0' && argv[optind][0] <= '9')
		return argv[optind++];
	return optarg;
}

// the input settings (-x, -r, -F) of every engine of the run: the plain one and both passes of -A
static void apply_input(gpu_engine &e, const job_settings &in)
{
	e.set_wide(in.wide);
	if (in.resampled())
		e.set_rate(in.rate_p, in.rate_q);
	e.set_format(in.fmt);
}

static bool parse_spec(const char *arg, spec &out)
{
	std::string a(arg);
	size_t pos = 0;
	for (;;) {
		const size_t e = a.find(',', pos);
		const std::string f = a.substr(pos, e == std::string::npos ? std::string::npos : e - pos);
		if (f.size() < 3 || f[1] != '=')
			return false;
		const char *v = f.c_str() + 2;
		if (f[0] == 'f') {
			if (out.freq >= 0 || !parse_khz(v, out.freq))
				return false;
			if (e == std::string::npos)
				return true;
			pos = e + 1;
			continue;
		}
		char *end = NULL;
		const long x = strtol(v, &end, f[0] == 'T' ? 16 : 10);
		if (*end || end == v)
			return false;
		if (f[0] == 'T' && out.types < 0 && x > 0 && (x & ~0x2fL) == 0)
			out.types = (int)x;
		else if (f[0] == 't' && out.thresh < 0 && x >= 0 && x <= 0x7fffffff)
			out.thresh = (int)x;
		else if (f[0] == 'W' && out.filter < 0 && (x == 0 || x == 1))
			out.filter = (int)x;
		else
			return false;  // unknown field, one given twice, or a value out of range (a mask outside 0x2f)
		if (e == std::string::npos)
			return true;
		pos = e + 1;
	}
}

static int replay_hex(int types, int dbg, const char *fn, const char *exec, bool batched)
{
	pipe_sink *psink = (batched && exec) ? new pipe_sink(exec) : NULL;
	batch_sink *sink = psink;
	std::vector<decoder *> decs = make_decoders(types, &sink, 0);
	decs.erase(std::remove(decs.begin(), decs.end(), (decoder *)NULL), decs.end());  // (the slots of types not asked for)
	FILE *fd = fopen(fn, "r");
	if (!fd) {
		perror("Can't open message file");
		return 1;
	}
	char line[2048];
	while (fgets(line, sizeof(line), fd)) {
		if (line[0] == '#')
			continue;
		uint8_t buf[512];
		int len = 0;
		for (char *tok = strtok(line, " \t\r\n"); tok && len < (int)sizeof(buf); tok = strtok(NULL, " \t\r\n"))
			buf[len++] = (uint8_t)strtol(tok, NULL, 16);
		for (size_t k = 0; k < decs.size(); k++) {
			decs[k]->set_params(batched ? NULL : (char *)exec, 0, dbg);
			decs[k]->store_bytes(buf, len);
			decs[k]->flush(0);
			puts("");
			decs[k]->flush_storage();
		}
	}
	fclose(fd);
	delete psink;  // flushes
	return 0;
}

// The command line, and main()'s steps over it in their order.  A step returns the exit code, or -1 to go on.
struct cli {
	int types = 0x07, thresh = 0, filter = 0, dbg = 0, blocks = 16;  // defaults of main.cpp:97-105 (0 = auto)
	std::vector<int> devices;
	std::vector<std::string> dumps;
	const char *hexfile = NULL, *exec = NULL;
	bool batched = false, bits = false, wide = false;
	int mode = 0, slots = 0;
	bool have_slots = false;
	spec cur;                     // the -p in force
	std::vector<spec> dump_spec;  // per -L file
	bool have_spec = false;
	long freq = -1, center = 868250;  // -f (unset: the dumps' own frequency), -c: kHz
	long rate = 0;  // -r: Hz (0: 1536000)
	int format = TFREC_AMD_FMT_U8;  // -F
	long scan_step = 0;  // -s: kHz
	bool have_scan = false;
	const char *cap_prefix = NULL;  // -S
	const char *replay_prefix = NULL;  // -R
	bool meter = false;  // -M
	bool envelope = false;  // -Q
	bool clock = false;  // -C
	long track_rate = 0, track_centre = 0;  // -G (rate 0: not given)
	bool track_centre_given = false;
	bool track_auto = false;  // -G rate,auto
	long track_lag = 0;  // -G rate,psk[,lag] (0: not given): m
	long track_level = -1;  // -O (-1: not given)
	int sync_bits = 0;  // -Y (0: not given): the word's bits, the word, errors, bytes, both
	unsigned long long sync_pattern = 0;
	long sync_errors = 0, sync_bytes = 8, sync_both = 0, sync_lsb = 0;
	uint32_t code_taps = 0;  // -U (0: not given): the taps and INVERT
	bool code_invert = false;
	int crc_width = 0, crc_skip = 0;  // -V (width 0: not given)
	uint32_t crc_poly = 0, crc_init = 0, crc_xorout = 0;
	bool crc_invert = false;
	const char *keep_prefix = NULL, *cont_prefix = NULL;  // -k, -K
	bool have_center = false, have_format = false;  // -c, -F given (-R refuses them)
	std::vector<replay_file> captures;  // -R: one per file index of <prefix>.idx
	int spec_bins = 0, spec_g = 0;  // -P (spec_g 0: the default)
	bool have_spec_p = false;
	bool have_auto = false;  // -A
	long auto_ratio = 32, auto_rel = 16, auto_join = 50;  // (join: kHz)
	// -z: the DC blocker's averaging length in windows of 512 input samples (0: off).  The default, 2048 windows = 0.68 s at
	// 1.536 MS/s, is derived from nothing but the burst lengths: an average much longer than any telegram (8 windows eat part of
	// a burst and lose a telegram, 64 do not: DESIGN.md 6m); it has not been measured on real recordings.
	long dc_windows = 0;
	// -Z: the IQ balancer's length in the same windows (0: off).  The default is -z's, by the same reasoning -- an estimate over much
	// more than a telegram, so that no single burst steers it; it has not been measured on real recordings either.
	long iq_windows = 0;
	job_settings in;                  // the input: -x, -r as P / Q, -F; it answers what follows from them (job.h)
	std::vector<long> scan_khz;       // -s, -A: the channels
	std::vector<file_settings> per_file;

	int parse(int argc, char **argv);
	bool parse_auto(const char *arg);
	bool parse_spectrum(const char *arg);
	bool parse_format(const char *arg);
	int check() const;
	int reduce_rate();
	int scan_channels();
	int tune_files();
	int find_channels();
	int load_capture();
	int run();
};

static void usage()
{
	fprintf(stderr, "usage: tfrec_gpu [-T hexmask] [-t thresh] [-W] [-f kHz] [-c kHz] [-x | -r Hz] [-F format] [-z [windows]] [-Z [windows]] [-q] [-D] [-B] [-d dev] [-b blocks] [-n streams] [-S prefix] [-M] [-Q] [-C] [-G rate[,centre_hz]] [-G rate,auto] [-G rate,psk[,lag]] [-O level] [-Y hex[,errors[,bytes[,both]]]] [-Y hex,errors,bytes,both,1] [-U g3ruh|nrzi|nrzs|hextaps[,inv]] [-V width,poly[,init[,xorout[,skip[,inv]]]]] [-k prefix] [-K prefix] [-p settings] -L dump [[-p settings] -L dump ...] | -s step_kHz -L dump | -P bins[,frames] -L dump | -A [ratio[,rel[,join_kHz]]] -L dump | -X hexfile\n"
			"  -A [r[,l[,j]]] find the occupied channels of one dump on the GPU (a bin's peak r times over the noise floor, default 32, and\n"
			"              within 1/l of the record's strongest, default 16; bins at most j kHz apart join, default 50), then scan those\n"
			"  -s kHz      scan one dump: a receiver every kHz step across it, a table of levels and telegrams per channel (-D: per block)\n"
			"  -P bins[,G] power spectrum of one dump beside its decoding: bins = 64 .. 1024 (a power of two), G frames per record; a\n"
			"              line per bin behind the telegrams (-D: per record too)\n"
			"  -S prefix   record the IQ of every trigger window: <prefix>.idx (a line per run) and <prefix>.<file>.cs16 (384 kS/s int16 I, Q)\n"
			"  -R prefix   replay a capture made by -S (<prefix>.idx, .cs16, .pre): decode its trigger windows again, with -T, -t, -d, -n, -b,\n"
			"              -D, -q, -e / -E; not with -L or anything that describes a dump\n"
			"  -M          measure every burst's carrier offset and FSK deviation on the GPU, decoded or not: a line 'burst <file>\n"
			"              <start_sample> <n_samples> <pwr_max> <centre_hz|-> <deviation_hz|->' per trigger window (-: no carrier); with -s or\n"
			"              -A a column burst_centre= of the channel's strongest burst instead; also with -R; not with -X\n"
			"  -Q          measure every burst's length, gaps and signal-to-noise ratio on the GPU, decoded or not: a line 'extent <file>\n"
			"              <start_sample> <n_samples> <burst_samples> <n_over> <n_gaps> <max_gap> <ratio|-> <snr_db|->' per trigger window\n"
			"              (-: no noise tail to compare with); with -s or -A a column burst_snr= of the channel's median ratio instead;\n"
			"              also with -M and -R; not with -X, -k or -K\n"
			"  -C          measure every burst's symbol rate on the GPU, decoded or not: a line 'clock <file> <start_sample> <n_samples>\n"
			"              <n_segments> <clock_hz|-> <quality|->' per trigger window (quality: the spectral peak over the band's mean; -: no\n"
			"              whole 1024-sample segment); with -s or -A a column burst_clock= of the channel's best-quality burst instead;\n"
			"              also with -M, -Q and -R; not with -X, -k or -K\n"
			"  -G r[,c]    read every burst's bits on the GPU, decoded or not, at r bit/s (1000 .. 96000) about the centre c Hz (default 0): a\n"
			"              line 'bits <file> <start_sample> <n_samples> <burst_samples> <n_bits>[+] <hex|->' per trigger window, MSB-first,\n"
			"              1 above the centre (+: longer than the 2^20 samples kept); also with -M, -Q, -C, -S and -R; not with -X, -k, -K,\n"
			"              -s or -A\n"
			"  -G r,auto   as -G r, every burst about a centre measured on its own first 1024 samples -- a recording of several transmitters\n"
			"              in one pass --, and ahead of each bits line a line 'centre <file> <start_sample> <n_samples> <n_counted> <centre_hz>\n"
			"              <deviation_hz|-> <m|f|i>' (m: measured; f: too few samples over the threshold, centre 0; i: inherited); not with -O\n"
			"  -G r,psk[,m] read phase-keyed bursts: the track is 1 where the phase is the one of m samples ago (1 .. 64; default a symbol,\n"
			"              (768000 + r) / (2 r)), about the burst's own carrier, measured on its first 1024 samples -- an NRZ-S transmitter's\n"
			"              bits --, and ahead of each bits line -G r,auto's centre line; not with -O\n"
			"  -O level    with -G r: read on-off keyed bursts: the track is 1 where the burst's amplitude (|I| + |Q|, -t's unit, smoothed as -G's)\n"
			"              lies above level (0 .. 65535; a place to start: half of -M's pwr_max); behind each bits line a line 'pulses <file>\n"
			"              <start_sample> <n_samples> <burst_samples> <n_pulses>[+] <w0,g0,w1,...|->', pulse and gap widths in samples (+: more\n"
			"              than the 64 pulses listed); no centre with it; works where -G works\n"
			"  -Y h[,e[,n[,b]]]  with -G: find the sync word h (2 .. 16 hex digits, MSB first) in every burst's track with at most e bit errors\n"
			"              (default 0), b = 1: or its complement, and read the n bytes behind it (default 8) at symbol centres: a line 'frame <file>\n"
			"              <start_sample> <sync_sample> <errors> <+|-> <n_bits> <hex|->' per match, behind the burst's bits line\n"
			"  -Y h,e,n,b,1  as -Y h,e,n,b, the frames' hex LSB-first per byte (the first received bit is bit 0; two digits a byte)\n"
			"  -U code[,inv] with -G: a line code ahead of the slicer and of -Y: g3ruh (descrambler, taps 12 and 17), nrzi, nrzs, or hex taps\n"
			"              (bit j - 1: the track XORed with itself j symbols ago), inv: complemented; behind each bits line a line 'code <file>\n"
			"              <start_sample> <n_samples> <burst_samples> <n_bits>[+] <hex|->', and -Y's frames are read from the coded track\n"
			"  -V w,p[,i[,x[,s[,v]]]]  with -G and -Y: check every frame's CRC on the GPU: width w (8, 16, 24, 32), poly p, init i and xorout x in\n"
			"              hex, s bytes skipped behind the sync word, v = 1: complemented bits; the frame is -Y's n bytes, the CRC its last w / 8:\n"
			"              every frame line ends in ok, bad or -, and behind them a line 'crc <file> <start_sample> <n_samples> <n_ok> <sample|->'\n"
			"  -k prefix   keep: for a recording that arrives in parts.  Every -L file is processed in whole blocks only (nothing is padded), then\n"
			"              its receiver's state is saved to <prefix>.<file index>.state and the bytes that filled no block to\n"
			"              <prefix>.<file index>.rest\n"
			"  -K prefix   continue: before it starts, every -L file's receiver is loaded from <prefix>.<file index>.state (this run's -T, -t\n"
			"              and -W must be the saved ones; the saved -f applies) and <prefix>.<file index>.rest is read ahead of the file's own bytes: the\n"
			"              telegrams of the parts, -k on one and -K on the next, are those of the whole recording, one that lies across two\n"
			"              parts included.  Same -T, -x, -r, -F, -z, -Z as the run that kept it.  Both may be given.  The host decoders' own\n"
			"              memory is not carried: the -m 1 table and the '#nnn' counter start again.  Not with -n, -s, -A, -P, -R, -S, -M, -X\n"
			"              or a path given to more than one -L\n"
			"  -f kHz      receive frequency (default: the dumps' own, -c)\n"
			"  -c kHz      frequency the dumps were recorded at (default 868250); -f within 767 kHz of it\n"
			"  -x          the dumps are 15.36 MS/s u8 dumps (10x the rate); -f within 7679 kHz of -c, shifted ahead of the 10:1 stage\n"
			"              (a file given to several -L is read once and shared by its streams; with -n it is read per -L, as before)\n"
			"  -r Hz       sample rate of the dumps (default 1536000), e.g. 2048000, 2400000 or any whole kHz such as 2500000 or 10000000\n"
			"              (between 1536000 and 15360000): resampled on the GPU; -b is rounded up\n"
			"              to a block count that holds a whole number of input samples; -f less than half the rate from -c (beyond\n"
			"              767 kHz it is shifted ahead of the resampler); not with -x\n"
			"  -F format   what the dumps hold: u8 (default), s8, s16 or f32 (cu8, cs8, cs16, cf32): little-endian interleaved I, Q without a\n"
			"              header, at the rate of -r or at 1536000; a format other than u8 not with -x\n"
			"  -z [n]      remove every dump's DC offset on the GPU, ahead of every tune: the mean over the last n windows of 512 input\n"
			"              samples (default 2048, within 1 .. 4096) is subtracted from I and from Q (-D: a 'dc' line per submit); not with\n"
			"              -x or -X; under -A the spectrum of pass 1 stays raw\n"
			"  -Z [n]      remove every dump's IQ imbalance (gain and phase error between I and Q, whose images decode as ghost transmitters)\n"
			"              on the GPU, behind -z and ahead of every tune: one correction per dump, estimated over the last n windows of 512\n"
			"              input samples (default 2048, within 1 .. 4096; -D: an 'iq' line per submit); use -z with it where the dump has a\n"
			"              DC offset; not with -x or -X\n"
			"  -n streams  at most this many streams per device: the -L files queue for them in order\n"
			"  -p T=<hex>,t=<n>,W=<0|1>,f=<kHz>  -T / -t / -W / -f of the -L files that follow, up to the next -p (fields left out: the global ones)\n");
}

bool cli::parse_auto(const char *arg)
{
	have_auto = true;
	long *field[3] = { &auto_ratio, &auto_rel, &auto_join };
	const long lo[3] = { 2, 1, 0 }, hi[3] = { 4096, 4096, 100000 };
	bool ok = true;
	const char *a = arg;
	for (int i = 0; a && ok; i++) {  // the fields between the commas, each a whole number in its range
		const char *comma = strchr(a, ',');
		const std::string f(a, comma ? (size_t)(comma - a) : strlen(a));
		ok = i < 3 && parse_long(f.c_str(), lo[i], hi[i], *field[i]);
		a = comma ? comma + 1 : NULL;
	}
	if (!ok)
		fprintf(stderr, "tfrec_gpu: bad -A '%s': want [ratio[,rel[,join_kHz]]], ratio within 2 .. 4096, rel within 1 .. 4096, "
				"join_kHz within 0 .. 100000\n", arg);
	return ok;
}

bool cli::parse_spectrum(const char *arg)
{
	const char *comma = strchr(arg, ',');
	long nb = 0, g = 0;
	have_spec_p = parse_long(std::string(arg, comma ? (size_t)(comma - arg) : strlen(arg)).c_str(), 64, 1024, nb) && (nb & (nb - 1)) == 0 &&
		      (!comma || parse_long(comma + 1, 1, 16384, g));
	spec_bins = (int)nb;
	spec_g = (int)g;
	if (!have_spec_p)
		fprintf(stderr, "tfrec_gpu: bad -P '%s': want <bins>[,<frames per record>], bins one of 64, 128, 256, 512, 1024, frames "
				"per record within 1 .. 16384\n", arg);
	return have_spec_p;
}

bool cli::parse_format(const char *arg)
{
	static const struct {
		const char *name;
		int fmt;
	} names[] = { { "u8", TFREC_AMD_FMT_U8 }, { "cu8", TFREC_AMD_FMT_U8 }, { "s8", TFREC_AMD_FMT_S8 }, { "cs8", TFREC_AMD_FMT_S8 },
		      { "s16", TFREC_AMD_FMT_S16 }, { "cs16", TFREC_AMD_FMT_S16 }, { "f32", TFREC_AMD_FMT_F32 }, { "cf32", TFREC_AMD_FMT_F32 } };
	format = -1;
	for (const auto &nm : names)
		if (!strcmp(arg, nm.name))
			format = nm.fmt;
	if (format < 0)
		fprintf(stderr, "tfrec_gpu: bad -F '%s': want u8, s8, s16 or f32 (cu8, cs8, cs16, cf32)\n", arg);
	return format >= 0;
}

int cli::parse(int argc, char **argv)
{
	int c;
	while ((c = getopt(argc, argv, "T:t:Wf:c:xr:F:qDBd:b:n:L:X:e:E:m:p:s:S:R:P:A::z::Z::MQCG:O:Y:U:V:k:K:h")) != -1) {
		switch (c) {
		case 'M': meter = true; break;
		case 'Q': envelope = true; break;
		case 'C': clock = true; break;
		case 'G': {
			const char *comma = strchr(optarg, ',');
			track_auto = comma && !strcmp(comma + 1, "auto");
			const bool psk = comma && !strncmp(comma + 1, "psk", 3) && (comma[4] == '\0' || comma[4] == ',');
			track_lag = 0;
			if (!parse_long(std::string(optarg, comma ? (size_t)(comma - optarg) : strlen(optarg)).c_str(), 1000, 96000, track_rate) ||
			    (comma && !track_auto && !psk && !parse_long(comma + 1, -192000, 192000, track_centre)) ||
			    (psk && comma[4] == ',' && !parse_long(comma + 5, 1, 64, track_lag))) {
				fprintf(stderr, "tfrec_gpu: bad -G '%s': want <rate>[,<centre_hz>], <rate>,auto or <rate>,psk[,<lag>], the rate within 1000 .. 96000 bit/s, "
						"the centre within -192000 .. 192000 Hz, the lag within 1 .. 64 samples\n", optarg);
				return 1;
			}
			if (psk && !track_lag) {  // a symbol in samples
				track_lag = (768000 + track_rate) / (2 * track_rate);
				if (track_lag > 64) {
					fprintf(stderr, "tfrec_gpu: bad -G '%s': a symbol at %ld bit/s is %ld samples, more than the lag's 64: give <rate>,psk,<lag>\n", optarg,
						track_rate, track_lag);
					return 1;
				}
			}
			track_centre_given = comma != NULL && !track_auto && !psk;
			if (track_auto || psk)
				track_centre = 0;
			break;
		}
		case 'O':
			if (!parse_long(optarg, 0, 65535, track_level)) {
				fprintf(stderr, "tfrec_gpu: bad -O '%s': want <level>, within 0 .. 65535 in -t's unit\n", optarg);
				return 1;
			}
			break;
		case 'Y': {
			std::vector<std::string> part(1);
			for (const char *q = optarg; *q; q++) {
				if (*q == ',')
					part.push_back("");
				else
					part.back() += *q;
			}
			const std::string &hex = part[0];
			bool ok = part.size() <= 5 && hex.size() >= 2 && hex.size() <= 16 && hex.find_first_not_of("0123456789abcdefABCDEF") == std::string::npos;
			if (ok) {
				sync_bits = 4 * (int)hex.size();
				sync_pattern = strtoull(hex.c_str(), NULL, 16);
				ok = (part.size() < 2 || parse_long(part[1].c_str(), 0, (sync_bits - 1) / 2, sync_errors)) &&
				     (part.size() < 3 || parse_long(part[2].c_str(), 1, 256, sync_bytes)) &&
				     (part.size() < 4 || parse_long(part[3].c_str(), 0, 1, sync_both)) &&
				     (part.size() < 5 || parse_long(part[4].c_str(), 1, 1, sync_lsb));  // (a flag: 1, or left out)
			}
			if (!ok) {
				fprintf(stderr, "tfrec_gpu: bad -Y '%s': want <hex>[,<errors>[,<bytes>[,<both>]]], 2 .. 16 hex digits, errors below half the word's "
						"bits, 1 .. 256 bytes, both 0 or 1; a fifth field is 1: LSB-first bytes\n", optarg);
				return 1;
			}
			break;
		}
		case 'U':
			if (!code_parse(optarg, code_taps, code_invert)) {
				fprintf(stderr, "tfrec_gpu: bad -U '%s': want g3ruh, nrzi, nrzs or 1 .. 8 hex digits of taps (not 0), each with an optional ,inv\n", optarg);
				return 1;
			}
			break;
		case 'V':
			if (!crc_parse(optarg, crc_width, crc_poly, crc_init, crc_xorout, crc_skip, crc_invert)) {
				fprintf(stderr, "tfrec_gpu: bad -V '%s': want <width>,<poly>[,<init>[,<xorout>[,<skip>[,<inv>]]]]: width 8, 16, 24 or 32, poly, init and "
						"xorout 1 .. 8 hex digits, skip a number, inv 0 or 1\n", optarg);
				return 1;
			}
			break;
		case 'k':
		case 'K':
			(c == 'k' ? keep_prefix : cont_prefix) = optarg;
			if (!*optarg) {
				fprintf(stderr, "tfrec_gpu: bad -%c '': want the prefix of the .state and .rest files\n", c);
				return 2;
			}
			break;
		case 'z': {
			const char *a = optional_arg(argc, argv);
			dc_windows = 2048;
			if (a && !parse_long(a, 1, 4096, dc_windows)) {
				fprintf(stderr, "tfrec_gpu: bad -z '%s': want the windows (of 512 input samples) the DC estimate averages over, within "
						"1 .. 4096\n", a);
				return 1;
			}
			break;
		}
		case 'Z': {
			const char *a = optional_arg(argc, argv);
			iq_windows = 2048;
			if (a && !parse_long(a, 1, 4096, iq_windows)) {
				fprintf(stderr, "tfrec_gpu: bad -Z '%s': want the windows (of 512 input samples) the IQ estimate runs over, within 1 .. 4096\n",
					a);
				return 1;
			}
			break;
		}
		case 'A':
			if (!parse_auto(optional_arg(argc, argv)))
				return 1;
			break;
		case 'P':
			if (!parse_spectrum(optarg))
				return 1;
			break;
		case 's':
			have_scan = true;
			if (!parse_long(optarg, 1, 100000000L, scan_step)) {
				fprintf(stderr, "tfrec_gpu: bad -s '%s': want the channel step in kHz, >= 1\n", optarg);
				return 1;
			}
			break;
		case 'S':
			cap_prefix = optarg;
			if (!*cap_prefix) {
				fprintf(stderr, "tfrec_gpu: bad -S '': want the prefix of the files to write\n");
				return 1;
			}
			break;
		case 'R':
			replay_prefix = optarg;
			if (!*replay_prefix) {
				fprintf(stderr, "tfrec_gpu: bad -R '': want the prefix of the capture to replay\n");
				return 2;
			}
			break;
		case 'T': types = (int)strtol(optarg, NULL, 16); break;
		case 't': thresh = atoi(optarg); break;
		case 'W': filter = 1; break;
		case 'f':
		case 'c':
			have_center = have_center || c == 'c';
			if (!parse_khz(optarg, c == 'f' ? freq : center)) {
				fprintf(stderr, "tfrec_gpu: bad -%c '%s': want a frequency in kHz\n", c, optarg);
				return 1;
			}
			break;
		case 'x': wide = true; break;
		case 'r':
			if (!parse_long(optarg, 1, 100000000L, rate)) {
				fprintf(stderr, "tfrec_gpu: bad -r '%s': want the dumps' sample rate in Hz\n", optarg);
				return 1;
			}
			break;
		case 'F':
			have_format = true;
			if (!parse_format(optarg))
				return 1;
			break;
		case 'q': dbg = -1; break;
		case 'D': dbg++; break;
		case 'B': bits = true; break;
		case 'd':  // one ordinal or a comma-separated list: the dump files are sharded over the devices by index
			for (char *tok = strtok(optarg, ","); tok; tok = strtok(NULL, ","))
				devices.push_back(atoi(tok));
			break;
		case 'b': blocks = atoi(optarg); break;
		case 'n': slots = atoi(optarg); have_slots = true; break;
		case 'L':
			dumps.push_back(optarg);
			dump_spec.push_back(cur);
			break;
		case 'p':
			cur = spec();
			have_spec = true;
			if (!parse_spec(optarg, cur)) {
				fprintf(stderr, "tfrec_gpu: bad -p '%s': want T=<hex mask within 2f>,t=<thresh >= 0>,W=<0|1>,f=<kHz>\n", optarg);
				return 1;
			}
			break;
		case 'X': hexfile = optarg; break;
		case 'e': exec = optarg; batched = false; break;
		case 'E': exec = optarg; batched = true; break;
		case 'm': mode = atoi(optarg); break;
		default:
			usage();
			return c == 'h' ? 0 : 1;
		}
	}
	return -1;
}

// what excludes what, before any file is looked at
int cli::check() const
{
	if (replay_prefix && (!dumps.empty() || wide || rate || have_format || freq >= 0 || have_center || have_scan || have_auto || have_spec_p ||
			      dc_windows || iq_windows || cap_prefix || have_spec || hexfile)) {
		fprintf(stderr, "tfrec_gpu: -R replays a capture, which is 384 kS/s int16 IQ and nothing else: not with -L, -x, -r, -F, -f, -c, -s, "
				"-A, -P, -z, -Z, -S, -p or -X\n");
		return 2;
	}
	if (keep_prefix || cont_prefix) {  // -k, -K: usage errors, before a device is opened
		if (have_slots || have_scan || have_auto || have_spec_p || replay_prefix || cap_prefix || meter || hexfile) {
			fprintf(stderr, "tfrec_gpu: -k and -K carry the receivers of -L files from one run to the next: not with -n, -s, -A, -P, -R, -S, "
					"-M or -X\n");
			return 2;
		}
		if (envelope) {
			fprintf(stderr, "tfrec_gpu: -k and -K do not carry a burst across runs: not with -Q\n");
			return 2;
		}
		if (clock) {
			fprintf(stderr, "tfrec_gpu: -k and -K do not carry a burst across runs: not with -C\n");
			return 2;
		}
		if (track_rate) {
			fprintf(stderr, "tfrec_gpu: -k and -K do not carry a burst across runs: not with -G\n");
			return 2;
		}
		for (size_t i = 0; i < dumps.size(); i++)
			for (size_t j = 0; j < i; j++)
				if (dumps[i] == dumps[j]) {
					fprintf(stderr, "tfrec_gpu: -k / -K: %s is given to more than one -L (a shared input's state is not kept)\n", dumps[i].c_str());
					return 2;
				}
		for (size_t i = 0; i < dumps.size() && cont_prefix; i++) {
			const std::string path = job_settings::kept_path(cont_prefix, i, ".state");
			FILE *f = fopen(path.c_str(), "rb");
			if (!f) {
				fprintf(stderr, "tfrec_gpu: -K: ");
				perror(path.c_str());
				return 2;
			}
			fclose(f);
		}
	}
	if (have_slots && slots < 1) {
		fprintf(stderr, "tfrec_gpu: -n must be >= 1\n");
		return 1;
	}
	if (have_scan && (have_slots || have_spec || freq >= 0 || exec || hexfile || dumps.size() > 1 || devices.size() > 1)) {
		fprintf(stderr, "tfrec_gpu: -s scans one -L file on one device: not with -n, -p, -f, -e, -E, -X, several -L or several -d\n");
		return 1;
	}
	if (have_spec_p && (have_scan || have_slots || have_spec || hexfile || dumps.size() > 1 || devices.size() > 1)) {
		fprintf(stderr, "tfrec_gpu: -P takes the spectrum of one -L file on one device: not with -s, -n, -p, -X, several -L or several -d\n");
		return 1;
	}
	if (have_auto && (have_scan || have_slots || have_spec || freq >= 0 || exec || hexfile || cap_prefix || dumps.size() > 1 || devices.size() > 1)) {
		fprintf(stderr, "tfrec_gpu: -A finds and scans the channels of one -L file on one device: not with -s, -n, -p, -f, -e, -E, -X, -S, "
				"several -L or several -d\n");
		return 1;
	}
	if (dc_windows && (wide || hexfile)) {
		fprintf(stderr, "tfrec_gpu: -z removes the DC offset of -L files at 1.536 MS/s or the rate of -r: not with -x or -X\n");
		return 1;
	}
	if (iq_windows && (wide || hexfile)) {
		fprintf(stderr, "tfrec_gpu: -Z removes the IQ imbalance of -L files at 1.536 MS/s or the rate of -r: not with -x or -X\n");
		return 1;
	}
	if (meter && hexfile) {
		fprintf(stderr, "tfrec_gpu: -M measures the bursts of -L files or of a capture (-R): not with -X\n");
		return 1;
	}
	if (envelope && hexfile) {
		fprintf(stderr, "tfrec_gpu: -Q measures the bursts of -L files or of a capture (-R): not with -X\n");
		return 1;
	}
	if (clock && hexfile) {
		fprintf(stderr, "tfrec_gpu: -C measures the bursts of -L files or of a capture (-R): not with -X\n");
		return 1;
	}
	if (track_level >= 0 && track_lag) {
		fprintf(stderr, "tfrec_gpu: -G rate,psk reads the phase track: not with -O, whose track is the amplitude's\n");
		return 1;
	}
	if (track_level >= 0 && track_auto) {
		fprintf(stderr, "tfrec_gpu: -G rate,auto centres the frequency track: not with -O, whose track is the amplitude's\n");
		return 1;
	}
	if (track_level >= 0 && (!track_rate || track_centre_given)) {
		fprintf(stderr, "tfrec_gpu: bad -O: it reads the amplitude track at the rate of -G: give -G rate with it, without a centre\n");
		return 1;
	}
	if (sync_bits && !track_rate) {
		fprintf(stderr, "tfrec_gpu: -Y finds its sync word in the track of -G: give -G rate[,centre_hz] with it\n");
		return 1;
	}
	if (sync_bits && (768000LL * (sync_bits - 1) + track_rate) / (2LL * track_rate) > 2047) {
		fprintf(stderr, "tfrec_gpu: -Y: %d bits at %ld bit/s span %lld samples, more than 2047\n", sync_bits, track_rate,
			(768000LL * (sync_bits - 1) + track_rate) / (2LL * track_rate));
		return 1;
	}
	if (code_taps && !track_rate) {
		fprintf(stderr, "tfrec_gpu: -U codes the track of -G: give -G rate[,centre_hz] with it\n");
		return 1;
	}
	if (code_taps && code_span(code_taps, track_rate) > 2047) {
		fprintf(stderr, "tfrec_gpu: -U: the taps %x at %ld bit/s span %llu samples, more than 2047\n", (unsigned)code_taps, track_rate,
			(unsigned long long)code_span(code_taps, track_rate));
		return 1;
	}
	if (crc_width && !(sync_bits && track_rate)) {
		fprintf(stderr, "tfrec_gpu: -V checks the frames of -Y: give -G rate and -Y hex,errors,bytes with it\n");
		return 1;
	}
	if (crc_width && sync_both) {
		fprintf(stderr, "tfrec_gpu: -V checks frames of polarity + alone: not with -Y's both\n");
		return 1;
	}
	if (crc_width) {
		const tfrec_crc::Settings s = { (int32_t)track_rate, (int32_t)sync_bytes, (int32_t)crc_skip, (int32_t)crc_width, crc_poly, crc_init, crc_xorout,
						(sync_lsb ? TFREC_AMD_CRC_LSB : 0u) | (crc_invert ? TFREC_AMD_CRC_INVERT : 0u) };
		if (const char *why = tfrec_crc::refusal(s)) {
			fprintf(stderr, "tfrec_gpu: -V: %s (%ld bit/s, %ld bytes: D = %lld)\n", why, track_rate, sync_bytes, tfrec_crc::reach(s));
			return 1;
		}
	}
	if (track_rate && (hexfile || have_scan || have_auto)) {
		fprintf(stderr, "tfrec_gpu: -G reads the bursts of -L files or of a capture (-R), a line per burst: not with -X, -s or -A\n");
		return 1;
	}
	if (cap_prefix && hexfile) {
		fprintf(stderr, "tfrec_gpu: -S records the trigger windows of -L files: not with -X\n");
		return 1;
	}
	if (have_spec && hexfile) {
		fprintf(stderr, "tfrec_gpu: -p applies to -L files, not to -X\n");
		return 1;
	}
	return -1;
}

// -r: the rate as P / Q of 1536000, checked by the library's own rules (no device needed); -b up to a permitted block count
int cli::reduce_rate()
{
	in.wide = wide;
	in.fmt = format;
	if (rate && wide) {
		fprintf(stderr, "tfrec_gpu: -r and -x exclude each other (-x is the fixed rate 15360000)\n");
		return 1;
	}
	if (format != TFREC_AMD_FMT_U8 && wide) {
		fprintf(stderr, "tfrec_gpu: -F and -x exclude each other (15.36 MS/s dumps are u8)\n");
		return 1;
	}
	if (rate && rate != 1536000) {
		long a = rate, b = 1536000;
		while (b) {
			const long t = a % b;
			a = b;
			b = t;
		}
		const long p = rate / a, q = 1536000 / a;
		if (p > 0x7fffffffL || tfrec_amd_resample_taps((int32_t)p, (int32_t)q, NULL, 0, NULL) != TFREC_AMD_OK) {
			fprintf(stderr, "tfrec_gpu: -r %ld: the rate is %ld/%ld of 1536000 S/s, which the resampler does not take (it needs "
					"1536000 < rate < 15360000 and a whole number of kHz or a denominator of at most 64, and refuses a few rates "
					"whose filter would be ambiguous or could overflow)\n", rate, p, q);
			return 1;
		}
		in.rate_p = (int)p;
		in.rate_q = (int)q;
		const int unit = in.unit();
		if (blocks >= 1 && blocks % unit) {
			const int up = (blocks + unit - 1) / unit * unit;
			fprintf(stderr, "tfrec_gpu: -b %d rounded up to %d: at %ld S/s a submit holds a multiple of %d blocks\n", blocks, up,
				rate, unit);
			blocks = up;
		}
	}
	return -1;
}

// -s: the file once per channel c + k * step, |k * step * 1000| <= fs_in / 2 - 192000 (in integers: 2000 |k| step <= fs_in - 384000)
int cli::scan_channels()
{
	const long fs_in = in.fs_in();
	const long kmax = (fs_in - 384000) / (2000 * scan_step);
	if (2 * kmax + 1 > 4096) {
		fprintf(stderr, "tfrec_gpu: -s %ld: %ld channels across the %ld S/s recording, at most 4096 are scanned at once\n", scan_step,
			2 * kmax + 1, fs_in);
		return 1;
	}
	const std::string path = dumps[0];
	dumps.clear();
	dump_spec.clear();
	for (long k = -kmax; k <= kmax; k++) {
		spec p;
		p.freq = center + k * scan_step;
		if (p.freq <= 0) {
			fprintf(stderr, "tfrec_gpu: -s: channel %ld kHz below zero: -c %ld is not the recording's frequency\n", p.freq, center);
			return 1;
		}
		dumps.push_back(path);
		dump_spec.push_back(p);
		scan_khz.push_back(p.freq);
	}
	return -1;
}

// every file's tune, checked before any device is opened, and the per-file settings the engine gets
int cli::tune_files()
{
	std::vector<int> tunes;
	bool tuned = false;
	for (const spec &p : dump_spec) {
		const long f = p.freq >= 0 ? p.freq : (freq >= 0 ? freq : center);
		const long lim = wide ? 7680 : 768;
		if (in.resampled()) {  // -r: |f - c| < fs_in / 2, that is 2 |f - c| Q < 1536 P in kHz
			if (2 * labs(f - center) * in.rate_q >= 1536L * in.rate_p) {
				fprintf(stderr, "tfrec_gpu: receive frequency %ld kHz (-f / -p f=) is %ld kHz from the dumps' %ld kHz (-c): less than "
						"%.1f kHz, half the %ld S/s band (-r), can be tuned\n", f, f - center, center, rate / 2000.0, rate);
				return 1;
			}
		} else if (f - center <= -lim || f - center >= lim) {
			fprintf(stderr, "tfrec_gpu: receive frequency %ld kHz (-f / -p f=) is %ld kHz from the dumps' %ld kHz (-c): at most "
					"%ld kHz, half the %s band, can be tuned%s\n", f, f - center, center, lim - 1,
				wide ? "15.36 MS/s" : "1.536 MS/s", wide ? "" : " (-x: 15.36 MS/s dumps, 7679 kHz)");
			return 1;
		}
		tunes.push_back((int)((f - center) * 1000));
		tuned = tuned || tunes.back() != 0;
	}
	if (have_spec || tuned || have_scan)
		for (size_t i = 0; i < dump_spec.size(); i++) {
			const spec &p = dump_spec[i];
			per_file.push_back(file_settings{ p.types >= 0 ? p.types : types, p.thresh >= 0 ? p.thresh : thresh,
							  p.filter >= 0 ? p.filter : filter, tunes[i] });
		}
	return -1;
}

// -A: pass 1, the file as one stream with the spectrum and the detector; then the channels it found become the files of a scan
int cli::find_channels()
{
	const int n_bins = have_spec_p ? spec_bins : 256;
	{
		gpu_engine e1(dumps, types, thresh, filter, dbg, devices, blocks);
		apply_input(e1, in);
		e1.set_spectrum(n_bins, spec_g ? spec_g : (int)std::max(1L, (long)in.input_samples(1) / n_bins), center);
		e1.set_occupancy((int)auto_ratio, (int)auto_rel, auto_join * 1000);
		const int rc1 = e1.run();
		fflush(stdout);
		if (rc1)
			return 2;
		scan_khz = e1.found_khz();
	}
	if (scan_khz.empty())
		return 0;
	// pass 2: the scan, on exactly those (each within the scan's own range, so within what can be tuned)
	const std::string path = dumps[0];
	dumps.clear();
	per_file.clear();
	for (long khz : scan_khz) {
		if (khz <= 0) {
			fprintf(stderr, "tfrec_gpu: -A: channel %ld kHz below zero: -c %ld is not the recording's frequency\n", khz, center);
			return 1;
		}
		dumps.push_back(path);
		per_file.push_back(file_settings{ types, thresh, filter, (int)((khz - center) * 1000) });
	}
	have_scan = true;
	have_spec_p = false;
	return -1;
}

// -R: <prefix>.idx, and per file index found in it <prefix>.<i>.cs16 and <prefix>.<i>.pre, read and checked before a device is opened
// -> the captures, in ascending file index, and their names as the job's files
int cli::load_capture()
{
	const std::string prefix(replay_prefix), idx_path = prefix + ".idx";
	FILE *idx = fopen(idx_path.c_str(), "r");
	if (!idx) {
		perror(idx_path.c_str());
		return 2;
	}
	std::map<int, replay_file> by_index;
	char line[256];
	for (long ln = 1; fgets(line, sizeof(line), idx); ln++) {
		int f = 0, thr = 0, used = 0;
		unsigned stream = 0, n = 0, flags = 0;
		long long start = 0;
		const char *why = NULL;
		if (sscanf(line, "%d %u %lld %u %d %u %n", &f, &stream, &start, &n, &thr, &flags, &used) != 6 || line[used])
			why = "want '<file index> <stream> <start_sample> <n_samples> <thresh> <flags>'";
		else if (f < 0 || start < 0 || n < 1)
			why = "a negative file index or start_sample, or an empty run";
		else {
			replay_file &rf = by_index[f];
			rf.index = f;
			const long long end = rf.runs.empty() ? 0 : rf.runs.back().start_sample + (long long)rf.runs.back().n_samples;
			if (start < end)
				why = "the run overlaps the file's run before it, or the file's runs are out of order";
			else {
				const tfrec_amd_run r = { stream, flags, start, n, thr,
							  (uint64_t)(rf.runs.empty() ? 0 : rf.runs.back().pool_offset + rf.runs.back().n_samples) };
				rf.runs.push_back(r);
			}
		}
		if (why) {
			fprintf(stderr, "%s:%ld: %s\n", idx_path.c_str(), ln, why);
			fclose(idx);
			return 2;
		}
	}
	fclose(idx);
	for (std::map<int, replay_file>::iterator it = by_index.begin(); it != by_index.end(); ++it) {
		replay_file &rf = it->second;
		const size_t pairs = (size_t)(rf.runs.back().pool_offset + rf.runs.back().n_samples);
		const struct {
			const char *ext;
			size_t want;
			std::vector<int16_t> *to;
		} parts[2] = { { ".cs16", pairs, &rf.pool }, { ".pre", rf.runs.size(), &rf.pre } };
		for (int k = 0; k < 2; k++) {
			const std::string path = prefix + "." + std::to_string(rf.index) + parts[k].ext;
			FILE *fp = fopen(path.c_str(), "rb");
			if (!fp) {
				perror(path.c_str());
				return 2;
			}
			parts[k].to->resize(2 * parts[k].want);
			const size_t got = fread(parts[k].to->data(), 4, parts[k].want, fp);
			fclose(fp);
			if (got != parts[k].want) {
				fprintf(stderr, "%s: %zu pairs, the lines of %s ask for %zu\n", path.c_str(), got, idx_path.c_str(), parts[k].want);
				return 2;
			}
		}
		dumps.push_back(prefix + "." + std::to_string(rf.index));
		captures.push_back(rf);
	}
	return -1;
}

int cli::run()
{
	gpu_engine e(dumps, types, thresh, filter, dbg, devices, blocks, per_file);
	if (replay_prefix)
		e.set_replay(captures);
	if (exec || mode)
		e.set_handler(exec, batched, mode);
	e.set_bits_replay(bits);
	e.set_slots(slots);
	apply_input(e, in);
	if (dc_windows)
		e.set_dc((int)dc_windows);
	if (iq_windows)
		e.set_iq((int)iq_windows);
	if (have_scan)
		e.set_scan(scan_khz);
	if (cap_prefix)
		e.set_capture(cap_prefix);
	if (meter)
		e.set_meter();
	if (envelope)
		e.set_envelope();
	if (clock)
		e.set_clock();
	if (track_rate)
		e.set_track(track_rate, track_centre);
	if (track_level >= 0)
		e.set_track_level(track_level);
	if (track_auto)
		e.set_track_auto();
	if (track_lag)
		e.set_track_phase((int)track_lag);
	if (sync_bits)
		e.set_sync(sync_pattern, sync_bits, (int)sync_errors, (int)sync_bytes, sync_both != 0, sync_lsb != 0);
	if (code_taps)
		e.set_code(code_taps, code_invert);
	if (crc_width)
		e.set_crc(crc_width, crc_poly, crc_init, crc_xorout, crc_skip, crc_invert);
	if (keep_prefix)
		e.set_keep(keep_prefix);
	if (cont_prefix)
		e.set_continue(cont_prefix);
	if (have_spec_p)  // the default record: the frames one block's input holds
		e.set_spectrum(spec_bins, spec_g ? spec_g : (int)std::max(1L, (long)in.input_samples(1) / spec_bins), center);
	int rc = e.run();
	fflush(stdout);
	return rc ? 2 : 0;
}

int main(int argc, char **argv)
{
	cli c;
	int r = c.parse(argc, argv);
	if (r < 0)
		r = c.check();
	if (r >= 0)
		return r;
	setvbuf(stdout, NULL, _IOFBF, 1 << 16);
	if (c.hexfile)
		return replay_hex(c.types, c.dbg, c.hexfile, c.exec, c.batched);
	if (c.replay_prefix && (r = c.load_capture()) >= 0)
		return r;
	if (c.dumps.empty()) {
		if (c.replay_prefix)  // (a capture without a run: nothing triggered, nothing to decode)
			return 0;
		fprintf(stderr, "tfrec_gpu: need -L <dumpfile>, -R <prefix> or -X <hexfile>\n");
		return 1;
	}
	if (c.thresh < 0) {
		fprintf(stderr, "tfrec_gpu: -t must be >= 0 (0 = auto)\n");
		return 1;
	}
	if ((r = c.reduce_rate()) >= 0 || (c.have_scan && (r = c.scan_channels()) >= 0) || (r = c.tune_files()) >= 0 ||
	    (c.have_auto && (r = c.find_channels()) >= 0))
		return r;
	return c.run();
}
