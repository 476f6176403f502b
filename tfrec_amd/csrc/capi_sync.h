// tfrec_amd/csrc/capi_sync.h -- the burst sync's entry points: included by capi.hip, which lists what is where.
#pragma once

constexpr int kSyncSpanLimit = 2047;  // the track bits a stream carries from submit to submit

int tfrec_amd_enable_burst_sync(tfrec_amd_ctx *c, int32_t rate, uint64_t pattern, int32_t n_bits, int32_t max_errors, uint32_t flags)
{
	if (!c)
		return TFREC_AMD_E_INVAL;
	if (rate < 1000 || rate > 96000) {
		snprintf(g_err, sizeof(g_err), "the burst sync's rate is within [1000, 96000] bit/s");
		return TFREC_AMD_E_INVAL;
	}
	if (n_bits < 8 || n_bits > 64) {
		snprintf(g_err, sizeof(g_err), "the burst sync's pattern has 8 .. 64 bits");
		return TFREC_AMD_E_INVAL;
	}
	if (max_errors < 0 || 2 * (long long)max_errors >= n_bits) {
		snprintf(g_err, sizeof(g_err), "the burst sync's errors are within 0 <= E < n_bits / 2");
		return TFREC_AMD_E_INVAL;
	}
	if (flags & ~TFREC_AMD_SYNC_BOTH) {
		snprintf(g_err, sizeof(g_err), "the burst sync's flags are 0 or 1, the complemented word too");
		return TFREC_AMD_E_INVAL;
	}
	const long long span = (768000LL * (n_bits - 1) + rate) / (2LL * rate);
	if (span > kSyncSpanLimit) {
		snprintf(g_err, sizeof(g_err), "the burst sync's pattern spans %lld samples at %d bit/s, more than %d", span, (int)rate, kSyncSpanLimit);
		return TFREC_AMD_E_INVAL;
	}
	if (!c->trk.on) {
		snprintf(g_err, sizeof(g_err), "the burst sync works on the burst track: call tfrec_amd_enable_burst_track first");
		return TFREC_AMD_E_INVAL;
	}
	if (c->syn.on) {
		snprintf(g_err, sizeof(g_err), "the burst sync is enabled already");
		return TFREC_AMD_E_INVAL;
	}
	TRY(check_live(c));
	if (c->submitted) {
		snprintf(g_err, sizeof(g_err), "the burst sync is enabled before the first submit");
		return TFREC_AMD_E_STATE;
	}
	HIPCHK(hipSetDevice(c->cfg.device));
	EnableGuard<BurstSync> guard(c, c->syn);
	BurstSync &o = c->syn;
	const size_t n = (size_t)c->cfg.n_streams;
	for (int k = 0; k < kSets; k++) {
		TRY(own_device(c, o.d_recs[k], (size_t)c->cap.max_runs * sizeof(tfrec_amd_burst_sync)));
		TRY(own_device(c, o.d_words[k], c->trk.n_words * sizeof(uint32_t)));
	}
	TRY(own_device(c, o.d_carry, n * 64 * sizeof(uint32_t)));
	TRY(own_device(c, o.d_hist, n * sizeof(uint32_t)));
	HIPCHK(hipMemset(o.d_carry, 0, n * 64 * sizeof(uint32_t)));  // (never used before a submit has written them: no first submit CONTINUES)
	HIPCHK(hipMemset(o.d_hist, 0, n * sizeof(uint32_t)));
	o.rate = rate;
	o.n_bits = n_bits;
	o.max_errors = max_errors;
	o.flags = flags;
	o.pattern = n_bits == 64 ? pattern : pattern & ((1ull << n_bits) - 1ull);
	o.on = guard.ok = true;
	return TFREC_AMD_OK;
}

int tfrec_amd_read_burst_syncs(tfrec_amd_ctx *c, tfrec_amd_burst_sync *out, size_t cap_runs, uint32_t *n_runs, uint32_t *words, size_t cap_words,
			       uint64_t *n_words)
{
	if (!c || !n_runs || !n_words || (cap_runs > 0 && !out) || (cap_words > 0 && !words))
		return TFREC_AMD_E_INVAL;
	if (!c->syn.on) {
		snprintf(g_err, sizeof(g_err), "the burst sync is off: call tfrec_amd_enable_burst_sync before the first submit");
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
	std::vector<tfrec_amd_burst_sync> tmp(have);
	if (have)
		HIPCHK(hipMemcpy(tmp.data(), c->syn.d_recs[set], have * sizeof(tfrec_amd_burst_sync), hipMemcpyDeviceToHost));
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
		snprintf(g_err, sizeof(g_err), "room for %zu sync records and %zu words, the submit delivers %zu and %llu", cap_runs, cap_words, have,
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
		HIPCHK(hipMemcpy(words, c->syn.d_words[set], (size_t)nw * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (have)
		memcpy(out, tmp.data(), have * sizeof(tfrec_amd_burst_sync));
	return overflow ? TFREC_AMD_E_OVERFLOW : TFREC_AMD_OK;
}
