// tfrec_amd/csrc/capi_decin.h -- channel-rate input: the constructor, the recorder's pre samples, sparse submits:
// included by capi.hip, which lists what is where.
#pragma once

int tfrec_amd_create_decimated(const tfrec_amd_config *cfg, tfrec_amd_ctx **out)
{
	if (!cfg || !out)
		return TFREC_AMD_E_INVAL;
	*out = nullptr;
	if (cfg->flags & TFREC_AMD_F_INPUT_10X) {
		snprintf(g_err, sizeof(g_err), "channel-rate input and the 15.36 MS/s input flag exclude each other");
		return TFREC_AMD_E_INVAL;
	}
	// 384 kS/s = 1536000 * 1 / 4, four bytes per pair: tfrec_amd_input_bytes gives n_blocks * 32768
	return create_with(cfg, InputSpec{ .fmt = TFREC_AMD_FMT_DEC16, .p = 1, .q = 4, .decimated = true }, out);
}

int tfrec_amd_enable_capture_pre(tfrec_amd_ctx *c)
{
	if (!c)
		return TFREC_AMD_E_INVAL;
	if (!c->cap.lane.on) {
		snprintf(g_err, sizeof(g_err), "the pre samples belong to the recorder: call tfrec_amd_enable_capture first");
		return TFREC_AMD_E_INVAL;
	}
	if (c->cap_pre.on) {
		snprintf(g_err, sizeof(g_err), "the recorder's pre samples are enabled already");
		return TFREC_AMD_E_INVAL;
	}
	TRY(check_live(c));
	if (c->submitted) {
		snprintf(g_err, sizeof(g_err), "the recorder's pre samples are enabled before the first submit");
		return TFREC_AMD_E_STATE;
	}
	HIPCHK(hipSetDevice(c->cfg.device));
	EnableGuard<CapturePre> guard(c, c->cap_pre);
	for (int k = 0; k < kSets; k++)
		TRY(own_device(c, c->cap_pre.d_pre[k], (size_t)c->cap.max_runs * sizeof(uint32_t)));
	c->cap_pre.on = guard.ok = true;
	return TFREC_AMD_OK;
}

int tfrec_amd_read_capture_pre(tfrec_amd_ctx *c, int16_t *pre, size_t cap_runs, uint32_t *n_runs)
{
	if (!c || !n_runs || (cap_runs > 0 && !pre))
		return TFREC_AMD_E_INVAL;
	if (!c->cap_pre.on) {
		snprintf(g_err, sizeof(g_err), "the recorder's pre samples are off: call tfrec_amd_enable_capture_pre before the first submit");
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
	size_t have = (size_t)std::min<unsigned long long>(hdr.n_runs, o.max_runs);
	if (overflow) {  // the prefix tfrec_amd_read_captures delivers: whole runs whose pairs the pool holds
		std::vector<tfrec_amd_run> &tmp = c->cap.tmp;
		tmp.resize(have);
		if (have)
			HIPCHK(hipMemcpy(tmp.data(), o.d_runs[set], have * sizeof(tfrec_amd_run), hipMemcpyDeviceToHost));
		size_t k = 0;
		while (k < have && tmp[k].pool_offset + tmp[k].n_samples <= o.max_samples)
			k++;
		have = k;
	}
	*n_runs = (uint32_t)std::min<unsigned long long>(hdr.n_runs, 0xffffffffull);
	if (cap_runs < have) {
		snprintf(g_err, sizeof(g_err), "room for %zu pre samples, the submit delivers %zu", cap_runs, have);
		return TFREC_AMD_E_INVAL;
	}
	if (have)
		HIPCHK(hipMemcpy(pre, c->cap_pre.d_pre[set], have * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return overflow ? TFREC_AMD_E_OVERFLOW : TFREC_AMD_OK;
}

int tfrec_amd_enable_runs_input(tfrec_amd_ctx *c, uint32_t max_runs, uint64_t max_samples)
{
	if (!c)
		return TFREC_AMD_E_INVAL;
	if (!c->input.channel()) {
		snprintf(g_err, sizeof(g_err), "sparse submits feed a channel-rate context (tfrec_amd_create_decimated)");
		return TFREC_AMD_E_INVAL;
	}
	if (max_runs == 0 || max_samples == 0 || max_runs > 0x7fffffffu) {
		snprintf(g_err, sizeof(g_err), "max_runs within [1, 2^31) and max_samples must not be 0");
		return TFREC_AMD_E_INVAL;
	}
	if (c->runs_in.on) {
		snprintf(g_err, sizeof(g_err), "sparse submits are enabled already");
		return TFREC_AMD_E_INVAL;
	}
	TRY(check_live(c));
	if (c->submitted) {
		snprintf(g_err, sizeof(g_err), "sparse submits are enabled before the first submit");
		return TFREC_AMD_E_STATE;
	}
	if (max_samples > (uint64_t)SIZE_MAX / sizeof(uint32_t)) {
		snprintf(g_err, sizeof(g_err), "max_samples too large");
		return TFREC_AMD_E_NOMEM;
	}
	HIPCHK(hipSetDevice(c->cfg.device));
	EnableGuard<RunsIn> guard(c, c->runs_in);
	RunsIn &o = c->runs_in;
	const size_t n = (size_t)c->cfg.n_streams;
	for (int k = 0; k < kSets; k++) {
		TRY(own_device(c, o.d_tab[k], (size_t)max_runs * sizeof(uint4)));
		TRY(own_pinned(c, o.h_tab[k], (size_t)max_runs * sizeof(uint4)));
		TRY(own_device(c, o.d_pool[k], (size_t)max_samples * sizeof(uint32_t)));
		TRY(own_pinned(c, o.h_pool[k], (size_t)max_samples * sizeof(uint32_t)));
		TRY(own_device(c, o.d_pre[k], (size_t)max_runs * sizeof(uint32_t)));
		TRY(own_pinned(c, o.h_pre[k], (size_t)max_runs * sizeof(uint32_t)));
		TRY(own_device(c, o.d_first[k], (n + 1) * sizeof(int32_t)));
		TRY(own_pinned(c, o.h_first[k], (n + 1) * sizeof(int32_t)));
		TRY(own_device(c, o.d_ov[k], n * sizeof(uint2)));
		TRY(own_pinned(c, o.h_ov[k], n * sizeof(uint2)));
	}
	o.max_runs = max_runs;
	o.max_samples = max_samples;
	o.on = guard.ok = true;
	return TFREC_AMD_OK;
}

// the rule list of tfrec_amd_submit_runs (tfrec_amd/decin.py: check restates it)
static int check_runs(const tfrec_amd_ctx *c, const tfrec_amd_run *runs, uint32_t n_runs, uint64_t n_pairs, int n_blocks)
{
	const long long M = (long long)n_blocks * kBlockDec;
	uint64_t total = 0;
	for (uint32_t i = 0; i < n_runs; i++) {
		const tfrec_amd_run &r = runs[i];
		const char *why = nullptr;
		if (r.stream >= (uint32_t)c->cfg.n_streams)
			why = "stream outside the context";
		else if (r.start_sample < 0 || r.start_sample >= M)
			why = "start_sample outside the submit";
		else if (r.n_samples < 1 || r.start_sample + (long long)r.n_samples > M)
			why = "n_samples is 0 or the run ends behind the submit";
		else if (r.pool_offset != total)
			why = "pool_offset is not the exclusive prefix sum of n_samples";
		else if (i > 0) {
			const tfrec_amd_run &p = runs[i - 1];
			if (r.stream < p.stream || (r.stream == p.stream && r.start_sample <= p.start_sample))
				why = "the table is not ordered by (stream, start_sample)";
			else if (r.stream == p.stream && r.start_sample < p.start_sample + (long long)p.n_samples + 1)
				why = "two runs of a stream overlap or touch: at least one sample lies between them";
		}
		if (why) {
			snprintf(g_err, sizeof(g_err), "run %u: %s", (unsigned)i, why);
			return TFREC_AMD_E_INVAL;
		}
		total += r.n_samples;
	}
	if (total != n_pairs) {
		snprintf(g_err, sizeof(g_err), "n_pairs %llu, the runs hold %llu", (unsigned long long)n_pairs, (unsigned long long)total);
		return TFREC_AMD_E_INVAL;
	}
	return TFREC_AMD_OK;
}

static int submit_runs_impl(tfrec_amd_ctx *c, const tfrec_amd_run *runs, uint32_t n_runs, const int16_t *samples, uint64_t n_pairs,
			    const int16_t *pre, int n_blocks)
{
	if (!c || n_blocks < 1 || n_blocks > c->cfg.max_blocks || (n_runs > 0 && (!runs || !pre)) || (n_pairs > 0 && !samples))
		return TFREC_AMD_E_INVAL;
	RunsIn &o = c->runs_in;
	if (!o.on) {
		snprintf(g_err, sizeof(g_err), "sparse submits are off: call tfrec_amd_enable_runs_input before the first submit");
		return TFREC_AMD_E_INVAL;
	}
	if (c->tunes.mapped) {
		snprintf(g_err, sizeof(g_err), "a mapped context takes dense submits only");
		return TFREC_AMD_E_INVAL;
	}
	if (n_runs > o.max_runs || n_pairs > o.max_samples) {
		snprintf(g_err, sizeof(g_err), "%u runs and %llu pairs, enabled for %u and %llu", (unsigned)n_runs, (unsigned long long)n_pairs,
			 (unsigned)o.max_runs, (unsigned long long)o.max_samples);
		return TFREC_AMD_E_INVAL;
	}
	TRY(check_runs(c, runs, n_runs, n_pairs, n_blocks));
	TRY(check_fifo(c));
	TRY(check_live(c));
	HIPCHK(hipSetDevice(c->cfg.device));
	const int set = (c->head + c->inflight) % kSets;  // the set's previous user has been drained: its staging is free
	const int n = c->cfg.n_streams;
	for (int s = 0; s <= n; s++)
		o.h_first[set][s] = 0;
	for (int s = 0; s < n; s++)
		o.h_ov[set][s] = make_uint2(0u, 0u);
	for (uint32_t i = 0; i < n_runs; i++) {
		const tfrec_amd_run &r = runs[i];
		const uint32_t start = (uint32_t)r.start_sample;
		o.h_tab[set][i] = make_uint4(start, start + r.n_samples, (uint32_t)r.pool_offset, (uint32_t)(r.pool_offset >> 32));
		o.h_first[set][r.stream + 1]++;
		uint32_t p;
		memcpy(&p, pre + 2 * (size_t)i, 4);
		o.h_pre[set][i] = p;
		if (start == 0 && !c->restart.marked[r.stream])  // its own predecessor; a stream that restarts here has none
			o.h_ov[set][r.stream] = make_uint2(1u, p);
	}
	for (int s = 0; s < n; s++)
		o.h_first[set][s + 1] += o.h_first[set][s];
	if (n_pairs)
		memcpy(o.h_pool[set], samples, (size_t)n_pairs * sizeof(uint32_t));
	hipStream_t fs = c->pipe[set].fs;
	if (n_runs) {
		HIPCHK(hipMemcpyAsync(o.d_tab[set], o.h_tab[set], (size_t)n_runs * sizeof(uint4), hipMemcpyHostToDevice, fs));
		HIPCHK(hipMemcpyAsync(o.d_pre[set], o.h_pre[set], (size_t)n_runs * sizeof(uint32_t), hipMemcpyHostToDevice, fs));
	}
	if (n_pairs)
		HIPCHK(hipMemcpyAsync(o.d_pool[set], o.h_pool[set], (size_t)n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice, fs));
	HIPCHK(hipMemcpyAsync(o.d_first[set], o.h_first[set], ((size_t)n + 1) * sizeof(int32_t), hipMemcpyHostToDevice, fs));
	HIPCHK(hipMemcpyAsync(o.d_ov[set], o.h_ov[set], (size_t)n * sizeof(uint2), hipMemcpyHostToDevice, fs));
	return submit_common(c, o.d_pool[set], 0, n_blocks, nullptr, true, true);
}

int tfrec_amd_submit_runs(tfrec_amd_ctx *c, const tfrec_amd_run *runs, uint32_t n_runs, const int16_t *samples, uint64_t n_pairs,
			  const int16_t *pre, int n_blocks)
{
	const auto t0 = std::chrono::steady_clock::now();
	const int rc = submit_runs_impl(c, runs, n_runs, samples, n_pairs, pre, n_blocks);
	if (c)
		c->hp_submit += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	return rc;
}
