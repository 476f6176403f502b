// tfrec_amd/csrc/capi_track.h -- the burst track's entry points: included by capi.hip, which lists what is where.
#pragma once

constexpr int kTrackCentreLimit = 192000;  // |hz| <= half the 384 kS/s channel rate

// r = floor((8192 hz + 384000) / 768000) mod 4096, a true floor (|hz| <= 192000: the numerator stays inside 32 bits' worth of 64)
static int32_t track_index(int32_t hz)
{
	const long long a = 8192LL * hz + 384000, b = 768000;
	const long long q = a / b - ((a % b) < 0 ? 1 : 0);
	return (int32_t)(q & 4095);
}

int tfrec_amd_enable_burst_track(tfrec_amd_ctx *c, int32_t smooth)
{
	if (!c)
		return TFREC_AMD_E_INVAL;
	if (smooth < 1 || smooth > 16) {
		snprintf(g_err, sizeof(g_err), "the burst track's smooth is within [1, 16]");
		return TFREC_AMD_E_INVAL;
	}
	if (!c->cap.lane.on) {
		snprintf(g_err, sizeof(g_err), "the burst track works on the recorder's table: call tfrec_amd_enable_capture first");
		return TFREC_AMD_E_INVAL;
	}
	if (c->trk.on) {
		snprintf(g_err, sizeof(g_err), "the burst track is enabled already");
		return TFREC_AMD_E_INVAL;
	}
	TRY(check_live(c));
	if (c->submitted) {
		snprintf(g_err, sizeof(g_err), "the burst track is enabled before the first submit");
		return TFREC_AMD_E_STATE;
	}
	HIPCHK(hipSetDevice(c->cfg.device));
	EnableGuard<BurstTrack> guard(c, c->trk);
	BurstTrack &o = c->trk;
	const size_t n = (size_t)c->cfg.n_streams;
	o.n_words = (size_t)((c->cap.max_samples + 31) >> 5);
	for (int k = 0; k < kSets; k++) {
		TRY(own_device(c, o.d_recs[k], (size_t)c->cap.max_runs * sizeof(tfrec_amd_track)));
		TRY(own_device(c, o.d_words[k], o.n_words * sizeof(uint32_t)));
		TRY(own_device(c, o.d_idx[k], n * sizeof(int32_t)));
		TRY(own_pinned(c, o.h_idx[k], n * sizeof(int32_t)));
	}
	TRY(own_device(c, o.d_carry, n * 16 * sizeof(uint32_t)));
	TRY(own_device(c, o.d_prior, n * sizeof(uint32_t)));
	HIPCHK(hipMemset(o.d_carry, 0, n * 16 * sizeof(uint32_t)));  // (never used before a submit has written them: no first submit CONTINUES)
	HIPCHK(hipMemset(o.d_prior, 0, n * sizeof(uint32_t)));
	o.idx.assign(n, 0);
	o.smooth = smooth;
	o.on = guard.ok = true;
	return TFREC_AMD_OK;
}

int tfrec_amd_set_burst_track_centre(tfrec_amd_ctx *c, const int32_t *streams, const int32_t *hz, int n)
{
	if (!c || n < 0 || (n > 0 && (!streams || !hz)))
		return TFREC_AMD_E_INVAL;
	if (!c->trk.on) {
		snprintf(g_err, sizeof(g_err), "the burst track is off: call tfrec_amd_enable_burst_track before the first submit");
		return TFREC_AMD_E_INVAL;
	}
	for (int i = 0; i < n; i++) {
		TRY(check_stream(c, streams[i]));
		if (hz[i] < -kTrackCentreLimit || hz[i] > kTrackCentreLimit) {
			snprintf(g_err, sizeof(g_err), "the burst track's centre %d Hz outside [-%d, %d]", (int)hz[i], kTrackCentreLimit, kTrackCentreLimit);
			return TFREC_AMD_E_INVAL;
		}
	}
	TRY(check_live(c));
	for (int i = 0; i < n; i++)
		c->trk.idx[streams[i]] = track_index(hz[i]);
	return TFREC_AMD_OK;
}

int tfrec_amd_read_burst_tracks(tfrec_amd_ctx *c, tfrec_amd_track *out, size_t cap_runs, uint32_t *n_runs, uint32_t *words, size_t cap_words,
				uint64_t *n_words)
{
	if (!c || !n_runs || !n_words || (cap_runs > 0 && !out) || (cap_words > 0 && !words))
		return TFREC_AMD_E_INVAL;
	if (!c->trk.on) {
		snprintf(g_err, sizeof(g_err), "the burst track is off: call tfrec_amd_enable_burst_track before the first submit");
		return TFREC_AMD_E_INVAL;
	}
	int set = 0;
	TRY(begin_side_read(c, c->cap.lane, "recorder", "call tfrec_amd_enable_capture before the first submit", &set));
	HIPCHK(hipSetDevice(c->cfg.device));
	HIPCHK(hipEventSynchronize(c->copied[set]));  // (behind the lane's written[set])
	const CaptureOut &o = c->cap;
	CaptureHeader hdr;
	HIPCHK(hipMemcpy(&hdr, o.d_hdr[set], sizeof(hdr), hipMemcpyDeviceToHost));
	const bool overflow = hdr.n_runs > o.max_runs || hdr.n_pairs > o.max_samples;
	// a record for every entry of the table; the words of the pairs tfrec_amd_read_captures delivers: on an overflow the prefix
	// of whole runs that fit the pool, found on the records' own bit_offset and n_samples
	const size_t have = (size_t)std::min<unsigned long long>(hdr.n_runs, o.max_runs);
	std::vector<tfrec_amd_track> tmp(have);
	if (have)
		HIPCHK(hipMemcpy(tmp.data(), c->trk.d_recs[set], have * sizeof(tfrec_amd_track), hipMemcpyDeviceToHost));
	uint64_t pairs = hdr.n_pairs;
	if (overflow) {
		pairs = 0;
		for (size_t k = 0; k < have && tmp[k].bit_offset + tmp[k].n_samples <= o.max_samples; k++)
			pairs = tmp[k].bit_offset + tmp[k].n_samples;
	}
	const uint64_t nw = (pairs + 31) >> 5;
	*n_runs = (uint32_t)std::min<unsigned long long>(hdr.n_runs, 0xffffffffull);
	*n_words = nw;
	if (cap_runs < have || (words && cap_words < nw)) {
		snprintf(g_err, sizeof(g_err), "room for %zu track records and %zu words, the submit delivers %zu and %llu", cap_runs, cap_words, have,
			 (unsigned long long)nw);
		return TFREC_AMD_E_INVAL;
	}
	if (!c->restart.set_origin[set].empty()) {  // start_sample counts from the stream's last restart, as the table's does
		const std::vector<long long> &org = c->restart.set_origin[set];
		for (size_t i = 0; i < have; i++)
			if (tmp[i].stream < org.size())
				tmp[i].start_sample -= org[tmp[i].stream];
	}
	if (words && nw)
		HIPCHK(hipMemcpy(words, c->trk.d_words[set], (size_t)nw * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (have)
		memcpy(out, tmp.data(), have * sizeof(tfrec_amd_track));
	return overflow ? TFREC_AMD_E_OVERFLOW : TFREC_AMD_OK;
}
