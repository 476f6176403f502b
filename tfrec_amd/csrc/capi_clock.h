// tfrec_amd/csrc/capi_clock.h -- the burst clock's entry points: included by capi.hip, which lists what is where.
#pragma once

int tfrec_amd_enable_burst_clock(tfrec_amd_ctx *c)
{
	if (!c)
		return TFREC_AMD_E_INVAL;
	if (!c->cap.lane.on) {
		snprintf(g_err, sizeof(g_err), "the burst clock works on the recorder's table: call tfrec_amd_enable_capture first");
		return TFREC_AMD_E_INVAL;
	}
	if (c->clk.on) {
		snprintf(g_err, sizeof(g_err), "the burst clock is enabled already");
		return TFREC_AMD_E_INVAL;
	}
	if (c->cfg.max_blocks >= 4096) {  // 8 segments a block: a record's device-side sums stay below 2^15 segments
		snprintf(g_err, sizeof(g_err), "the burst clock needs max_blocks < 4096");
		return TFREC_AMD_E_INVAL;
	}
	TRY(check_live(c));
	if (c->submitted) {
		snprintf(g_err, sizeof(g_err), "the burst clock is enabled before the first submit");
		return TFREC_AMD_E_STATE;
	}
	HIPCHK(hipSetDevice(c->cfg.device));
	EnableGuard<BurstClock> guard(c, c->clk);
	for (int k = 0; k < kSets; k++)
		TRY(own_device(c, c->clk.d_recs[k], (size_t)c->cap.max_runs * sizeof(tfrec_amd_clock)));
	c->clk.on = guard.ok = true;
	return TFREC_AMD_OK;
}

int tfrec_amd_read_burst_clocks(tfrec_amd_ctx *c, tfrec_amd_clock *out, size_t cap_runs, uint32_t *n_runs)
{
	if (!c || !n_runs || (cap_runs > 0 && !out))
		return TFREC_AMD_E_INVAL;
	if (!c->clk.on) {
		snprintf(g_err, sizeof(g_err), "the burst clock is off: call tfrec_amd_enable_burst_clock before the first submit");
		return TFREC_AMD_E_INVAL;
	}
	int set = 0;
	TRY(begin_side_read(c, c->cap.lane, "recorder", "call tfrec_amd_enable_capture before the first submit", &set));
	HIPCHK(hipSetDevice(c->cfg.device));
	HIPCHK(hipEventSynchronize(c->copied[set]));  // (behind the lane's written[set])
	CaptureHeader hdr;
	HIPCHK(hipMemcpy(&hdr, c->cap.d_hdr[set], sizeof(hdr), hipMemcpyDeviceToHost));
	// every entry of the table has a record, whatever the pool held: the kernels read the decimated samples
	const size_t have = (size_t)std::min<unsigned long long>(hdr.n_runs, c->cap.max_runs);
	*n_runs = (uint32_t)std::min<unsigned long long>(hdr.n_runs, 0xffffffffull);
	if (cap_runs < have) {
		snprintf(g_err, sizeof(g_err), "room for %zu clock records, the submit delivers %zu", cap_runs, have);
		return TFREC_AMD_E_INVAL;
	}
	if (have)
		HIPCHK(hipMemcpy(out, c->clk.d_recs[set], have * sizeof(tfrec_amd_clock), hipMemcpyDeviceToHost));
	if (!c->restart.set_origin[set].empty()) {  // start_sample counts from the stream's last restart, as the table's does
		const std::vector<long long> &org = c->restart.set_origin[set];
		for (size_t i = 0; i < have; i++)
			if (out[i].stream < org.size())
				out[i].start_sample -= org[out[i].stream];
	}
	return hdr.n_runs > c->cap.max_runs ? TFREC_AMD_E_OVERFLOW : TFREC_AMD_OK;
}
