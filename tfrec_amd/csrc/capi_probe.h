// tfrec_amd/csrc/capi_probe.h -- probes, read-backs, statistics: included by capi.hip, which lists what is where.
#pragma once

// The discriminator samples the device decided with its exact slow path (fm_resolve.h), checked against the libm of
// THIS host -- the arithmetic the reference binary would use here (dsp_stuff.cpp:284-292 as compiled: DESIGN.md 1).
static void account_fm_log(FmTotals *t, const EventBuf &eb)
{
	t->resolved += eb.uncertain;
	t->undecidable += eb.fm_undecidable;
	const uint32_t n = std::min<uint32_t>(eb.fm_logged, (uint32_t)kFmLogCap);
	const double scale = 16384.0 * (1.0 / M_PI);
	for (uint32_t k = 0; k < n; k++) {
		const int want = d2i_host(atan2(eb.fm_log[k].cj, eb.fm_log[k].cr) * scale);
		t->verified++;
		if (want != eb.fm_log[k].result)
			t->mismatch++;
	}
}

// Instrumentation builds and knobs: statistics of the third submit, printed to stderr (the host waits for the device first)
static void report_debug_stats(tfrec_amd_ctx *c, int set, int n_blocks)
{
#ifdef TFREC_AMD_VECSTAT
	if (c->submit_seq == 3) {
		(void)hipDeviceSynchronize();
		unsigned long long st[16] = { 0 };
		(void)hipMemcpy(st, c->win[set].stats, sizeof(st), hipMemcpyDeviceToHost);
		fprintf(stderr, "VECSTAT (one submit) TFA_1: groups %llu, stale piece %llu, entered-with-none hazard %llu, > 64 bits in a lane %llu, lanes with 32 ones or more %llu; TFA_2 family: groups %llu, entered with relative 0 %llu, > 16 rounds %llu, > 64 bits in a lane %llu, walks of the groups that converged %llu\n", st[8], st[9], st[10], st[11], st[5], st[12], st[13], st[14], st[15], st[6]);
	}
#endif
#ifdef TFREC_AMD_COOPSTAT
	if (c->submit_seq == 3) {
		(void)hipDeviceSynchronize();
		unsigned long long st[16] = { 0 };
		(void)hipMemcpy(st, c->win[set].stats, sizeof(st), hipMemcpyDeviceToHost);
		fprintf(stderr, "COOPSTAT (one submit) TFA_2 family: frozen one-block steps %llu, accepted %llu, rejected %llu, other frozen steps %llu; TFA_1: steps %llu, candidate runs %llu; TFA_2 walked steps with a full mask %llu, candidates in walked steps %llu, walked steps that begin inside a run %llu\n", st[7], st[8], st[9], st[10], st[11], st[12], st[13], st[14], st[15]);
	}
#endif
	if (TFREC_KNOB_STR("DEBUG_WINHIST") && c->submit_seq == 3) {  // (debug: the window length distribution of one submit)
		(void)hipDeviceSynchronize();
		const WinTables &T = c->win[set];
		const size_t chains = (size_t)c->launch.n_active * c->cfg.n_streams;
		std::vector<int32_t> cnt(chains), op(chains * T.cap), cl(chains * T.cap);
		(void)hipMemcpy(cnt.data(), T.count, chains * 4, hipMemcpyDeviceToHost);
		(void)hipMemcpy(op.data(), T.open, chains * T.cap * 4, hipMemcpyDeviceToHost);
		(void)hipMemcpy(cl.data(), T.close, chains * T.cap * 4, hipMemcpyDeviceToHost);
		const int M = n_blocks * kBlockDec;
		for (int a = 0; a < c->launch.n_active; a++) {
			long hist[16] = { 0 }, nwin = 0, tot = 0;
			for (int s = 0; s < c->cfg.n_streams; s++) {
				const size_t ch = (size_t)a * c->cfg.n_streams + s;
				for (int j = 0; j < cnt[ch]; j++) {
					const int last = cl[ch * T.cap + j] < M ? cl[ch * T.cap + j] : M - 1;
					const int n = last - op[ch * T.cap + j] + 1;
					int b = 0;
					while ((256 << b) <= n && b < 15)
						b++;
					hist[b]++;
					nwin++;
					tot += n;
				}
			}
			fprintf(stderr, "WINHIST slot %d kind %d window %d: %ld windows, %ld samples (%.1f %% of the submit);", a, c->launch.params[a].kind,
				c->launch.params[a].window, nwin, tot, 100.0 * tot / ((double)M * c->cfg.n_streams));
			for (int b = 0; b < 16; b++)
				if (hist[b])
					fprintf(stderr, " <%d:%ld", 256 << b, hist[b]);
			fprintf(stderr, "\n");
		}
	}
	if (TFREC_KNOB_STR("DEBUG_CONVHIST") && c->submit_seq == 3 && !(c->cfg.flags & TFREC_AMD_F_SERIAL_CHAINS)) {
		// (debug: after how many 32-sample slots the first repair run of a biquad segment -- started from the end state of the
		// segment before -- became bit-identical to the segment's own run from a zero state: the convergence-time distribution
		// of the speculation, per chain; a build with -DTFREC_AMD_CK_EVERY=1 resolves it to one slot)
		(void)hipDeviceSynchronize();
		const WinTables &T = c->win[set];
		const size_t chains = (size_t)c->launch.n_active * c->cfg.n_streams;
		std::vector<int32_t> fx(chains * T.segcap), vt(chains);
		(void)hipMemcpy(fx.data(), T.segfix, fx.size() * 4, hipMemcpyDeviceToHost);
		(void)hipMemcpy(vt.data(), T.vtotal, chains * 4, hipMemcpyDeviceToHost);
		for (int a = 0; a < c->launch.n_active; a++) {
			if (c->launch.params[a].kind == 0)
				continue;
			std::vector<long> hist(kSegSlots + 1, 0);
			long nseg = 0, never = 0;
			for (int s = 0; s < c->cfg.n_streams; s++) {
				const size_t ch = (size_t)a * c->cfg.n_streams + s;
				const int ns = (vt[ch] + kSegSlots - 1) / kSegSlots;
				for (int k = 1; k < ns; k++) {
					if (vt[ch] - k * kSegSlots < kSegSlots)
						continue;  // (a chain's short last segment says nothing)
					const int v = fx[ch * T.segcap + k];
					nseg++;
					if (v & kSegConverged)
						hist[std::min(kSegSlots, v & ~(kSegConverged | kSegRan))]++;
					else
						never++;
				}
			}
			fprintf(stderr, "CONVHIST slot %d (window %d, segments of %d slots): %ld full segments, %ld not converged at their end; converged within n slots:",
				c->launch.slot[a], c->launch.params[a].window, kSegSlots, nseg, never);
			long cum = 0;
			for (int n = 1; n <= kSegSlots; n++) {
				cum += hist[n];
				if (n == 4 || n == 8 || n == 12 || n == 16 || n == 20 || n == 24 || n == 32 || n == 40 || n == 48 || n == 64 || n == 96 ||
				    n == 128 || n == 192 || n == 256 || n == 384 || n == 512 || n == 1024)
					fprintf(stderr, " %d:%.4f", n, nseg ? (double)cum / nseg : 0.0);
			}
			fprintf(stderr, "\n");
		}
	}
}

int tfrec_amd_read_stage0(tfrec_amd_ctx *c, int stream, int16_t *out, size_t n_pairs)
{
	if (!c || !out || !c->input.in16() || stream < 0 || stream >= c->cfg.n_streams ||
	    n_pairs > (size_t)c->last_blocks * 4 * kBlockDec)
		return TFREC_AMD_E_INVAL;
	TRY(tfrec_amd_sync(c));
	HIPCHK(hipMemcpy(out, c->input.d_in16[c->last_set] + (size_t)stream * c->input.in16_stride, n_pairs * sizeof(uint32_t),
			 hipMemcpyDeviceToHost));
	return TFREC_AMD_OK;
}

int tfrec_amd_read_decimated(tfrec_amd_ctx *c, int stream, int16_t *out, size_t n_pairs)
{
	if (!c || !out || stream < 0 || stream >= c->cfg.n_streams || n_pairs > (size_t)c->last_blocks * kBlockDec)
		return TFREC_AMD_E_INVAL;
	TRY(tfrec_amd_sync(c));
	HIPCHK(hipMemcpy(out, c->d_dec[c->last_set] + (size_t)stream * c->dec_stride, n_pairs * sizeof(uint32_t),
			 hipMemcpyDeviceToHost));
	return TFREC_AMD_OK;
}

int tfrec_amd_read_biquad_row(tfrec_amd_ctx *c, int slot, int stream, int32_t *out, size_t cap_values, uint32_t *n_slots)
{
	if (!c || !n_slots || stream < 0 || stream >= c->cfg.n_streams || (c->cfg.flags & TFREC_AMD_F_SERIAL_CHAINS) ||
	    c->last_drained < 0 || (!out && cap_values))
		return TFREC_AMD_E_INVAL;
	int a = -1;
	for (int k = 0; k < c->launch.n_active; k++)
		if (c->launch.slot[k] == slot && c->launch.params[k].kind > 0)  // (TFA_1 has no biquad stage)
			a = k;
	if (a < 0)
		return TFREC_AMD_E_INVAL;
	const int set = c->last_drained;
	const WinTables &T = c->win[set];
	const size_t n = (size_t)T.slots * 32;
	if (out && cap_values < n)
		return TFREC_AMD_E_INVAL;
	*n_slots = (uint32_t)T.slots;
	if (!out)
		return TFREC_AMD_OK;
	TRY(tfrec_amd_sync(c));
	if (c->launch.params[a].kind == 2) {
		HIPCHK(hipMemcpy(out, c->d_dev32[set] + (size_t)stream * n, n * sizeof(int32_t), hipMemcpyDeviceToHost));
	} else {
		std::vector<int16_t> row(n);
		const size_t ch = (size_t)a * c->cfg.n_streams + stream - (size_t)T.ld_c0;
		HIPCHK(hipMemcpy(row.data(), c->d_ld16[set] + ch * n, n * sizeof(int16_t), hipMemcpyDeviceToHost));
		for (size_t k = 0; k < n; k++)
			out[k] = row[k];
	}
	return TFREC_AMD_OK;
}

int tfrec_amd_atan_uncertain(tfrec_amd_ctx *c, uint64_t *n)
{
	if (!c || !n)
		return TFREC_AMD_E_INVAL;
	if (c->poisoned)
		return TFREC_AMD_E_STATE;
	TRY(tfrec_amd_sync(c));
	*n = c->fm.resolved;
	for (int k = 0; k < c->inflight; k++) {  // submits not drained yet
		EventBuf eb;
		HIPCHK(hipMemcpy(&eb, c->d_eb[(c->head + k) % kSets], sizeof(eb), hipMemcpyDeviceToHost));
		*n += eb.uncertain;
	}
	return TFREC_AMD_OK;
}

int tfrec_amd_get_fm_stats(tfrec_amd_ctx *c, tfrec_amd_fm_stats *out)
{
	if (!c || !out)
		return TFREC_AMD_E_INVAL;
	if (c->poisoned)
		return TFREC_AMD_E_STATE;
	memset(out, 0, sizeof(*out));
	out->resolved = c->fm.resolved;
	out->host_verified = c->fm.verified;
	out->host_mismatch = c->fm.mismatch;
	out->undecidable = c->fm.undecidable;
	return TFREC_AMD_OK;
}

int tfrec_amd_fm_dev_probe(int device, int kind, const void *quads_v, size_t n, int32_t *out, tfrec_amd_fm_stats *stats)
{
	const int32_t *quads = (const int32_t *)quads_v;
	if (!quads || !out || n == 0 || n > (1u << 26) || kind < 0 || kind > 2)
		return TFREC_AMD_E_INVAL;
	HIPCHK(hipSetDevice(device));
	int32_t *d_q = nullptr, *d_o = nullptr;
	EventBuf *d_eb = nullptr;
	int rc = TFREC_AMD_OK;
	FmTotals tmp;
	if (hipMalloc((void **)&d_q, n * 16) != hipSuccess || hipMalloc((void **)&d_o, n * 4) != hipSuccess ||
	    hipMalloc((void **)&d_eb, sizeof(EventBuf)) != hipSuccess)
		rc = TFREC_AMD_E_NOMEM;
	// In pieces, so that the log (the first kFmLogCap slow-path decisions of a launch) does not saturate early; a caller
	// that wants EVERY sample checked compares `out` with its own reference.
	const size_t piece = 4096;
	if (rc == TFREC_AMD_OK && hipMemcpy(d_q, quads, n * 16, hipMemcpyHostToDevice) != hipSuccess)
		rc = TFREC_AMD_E_HIP;
	for (size_t o = 0; o < n && rc == TFREC_AMD_OK; o += piece) {
		const size_t m = std::min(piece, n - o);
		EventBuf eb;
		if (hipMemset(d_eb, 0, sizeof(EventBuf)) != hipSuccess || launch_fm_probe(nullptr, d_q + 4 * o, m, d_o + o, d_eb, kind) != hipSuccess ||
		    hipMemcpy(&eb, d_eb, sizeof(eb), hipMemcpyDeviceToHost) != hipSuccess)
			rc = hip_fail(hipGetLastError(), "fm_probe");
		else
			account_fm_log(&tmp, eb);
	}
	if (rc == TFREC_AMD_OK && hipMemcpy(out, d_o, n * 4, hipMemcpyDeviceToHost) != hipSuccess)
		rc = TFREC_AMD_E_HIP;
	(void)hipFree(d_q);
	(void)hipFree(d_o);
	(void)hipFree(d_eb);
	if (stats) {
		memset(stats, 0, sizeof(*stats));
		stats->resolved = tmp.resolved;
		stats->host_verified = tmp.verified;
		stats->host_mismatch = tmp.mismatch;
		stats->undecidable = tmp.undecidable;
	}
	return rc;
}

int tfrec_amd_iir_probe(int device, double cutoff, int form, const double *in, size_t n, double *out)
{
	if (!in || !out || n == 0 || n > (1u << 24) || form < 0 || form > 1 || !(cutoff > 0.0 && cutoff < 0.5))
		return TFREC_AMD_E_INVAL;
	HIPCHK(hipSetDevice(device));
	double *d_in = nullptr, *d_out = nullptr;
	int rc = TFREC_AMD_OK;
	if (hipMalloc((void **)&d_in, n * 8) != hipSuccess || hipMalloc((void **)&d_out, n * 8) != hipSuccess)
		rc = TFREC_AMD_E_NOMEM;
	if (rc == TFREC_AMD_OK && (hipMemcpy(d_in, in, n * 8, hipMemcpyHostToDevice) != hipSuccess ||
				   launch_iir_probe(nullptr, d_in, n, biquad_coef(cutoff), d_out, form) != hipSuccess ||
				   hipMemcpy(out, d_out, n * 8, hipMemcpyDeviceToHost) != hipSuccess))
		rc = hip_fail(hipGetLastError(), "iir_probe");
	(void)hipFree(d_in);
	(void)hipFree(d_out);
	return rc;
}

int tfrec_amd_read_thresh(tfrec_amd_ctx *c, int stream, int *thresh)
{
	if (!c || !thresh || stream < 0 || stream >= c->cfg.n_streams)
		return TFREC_AMD_E_INVAL;
	if (!c->settings.per_stream && c->cfg.thresh) {  // (a configured stream's FskState holds its fixed threshold: stream_reset_kernel)
		*thresh = c->cfg.thresh;
		return TFREC_AMD_OK;
	}
	TRY(tfrec_amd_sync(c));
	FskState f;
	HIPCHK(hipMemcpy(&f, c->d_fsk + stream, sizeof(f), hipMemcpyDeviceToHost));
	*thresh = f.thresh;
	return TFREC_AMD_OK;
}

int tfrec_amd_get_timings(tfrec_amd_ctx *c, tfrec_amd_timings *out)
{
	if (!c || !out)
		return TFREC_AMD_E_INVAL;
	if (!c->timed)
		return TFREC_AMD_E_STATE;
	// the most recently drained submit; before the first drain: the oldest one in flight
	const int set = c->last_drained >= 0 ? c->last_drained : c->head;
	hipEvent_t *ev = c->ev[set], *tev = c->tev[set];
	for (hipEvent_t e : c->pipe[set].done)
		HIPCHK(hipEventSynchronize(e));
	HIPCHK(hipEventElapsedTime(&out->frontend_ms, ev[kEvSubmit], ev[kEvFrontDone]));
	if (TFREC_KNOB_STR("HOST_PROF") && c->hp_n > 2) {  // idle time of the front-end stream between two submits' front ends
		float gap = 0, total = 0;
		const int next = (set + 1) % kSets;  // (in flight: its front end started long ago)
		if (hipEventElapsedTime(&gap, ev[kEvFrontDone], c->ev[next][kEvSubmit]) == hipSuccess &&
		    hipEventElapsedTime(&total, ev[kEvSubmit], tev[kMarkTfa1End]) == hipSuccess &&
		    gap > -1000 && gap < 1000) {
			float s2s = 0;
			if (hipEventElapsedTime(&s2s, ev[kEvSubmit], c->ev[next][kEvSubmit]) == hipSuccess)
				c->hp_s2s += s2s;
			c->hp_gap += gap;
			c->hp_lat += total;
			c->hp_gap_n++;
		}
		(void)hipGetLastError();
	}
	HIPCHK(hipEventElapsedTime(&out->fmdev_ms, ev[kEvFrontDone], ev[kEvFmdevDone]));
	if (c->fmdev_k2)  // (the discriminator pass ran in the pipeline)
		HIPCHK(hipEventElapsedTime(&out->fmdev_ms, tev[kMarkFmdev], tev[kMarkFmdevEnd]));
	out->windows_ms = out->spec_biquad_ms = out->repair_biquad_ms = out->fix_biquad_ms = out->slicer_ms = 0;
	out->coop_slicer_ms = out->decode_ms = out->commit_ms = 0;
	out->whb_biquad_ms = out->whb_demod_ms = out->whb_decode_ms = out->whb_commit_ms = 0;
	out->tfa1_slicer_ms = out->tfa1_coop_slicer_ms = out->tfa1_decode_commit_ms = 0;
	out->whb_verify_ms = 0;
	if (c->cfg.flags & TFREC_AMD_F_SERIAL_CHAINS) {
		HIPCHK(hipEventElapsedTime(&out->chains_ms, ev[kEvFmdevDone], ev[kEvSerialDone]));
		HIPCHK(hipEventElapsedTime(&out->total_ms, ev[kEvSubmit], ev[kEvSerialDone]));
		return TFREC_AMD_OK;
	}
	// the submit ends when the last of its three chains does
	out->chains_ms = out->total_ms = 0;
	const bool has_tfa2 = has_kind(c->launch, 1), has_whb = has_kind(c->launch, 2), has_tfa1 = has_kind(c->launch, 0);
	const struct {
		bool has;
		int end;
	} chain_end[3] = { { has_tfa2, kMarkTfa2End }, { has_whb, kMarkWhbCommitEnd }, { has_tfa1, kMarkTfa1End } };
	for (const auto &ce : chain_end)
		if (ce.has) {
			float t = 0;
			HIPCHK(hipEventElapsedTime(&t, ev[kEvFmdevDone], tev[ce.end]));
			out->chains_ms = std::max(out->chains_ms, t);
			HIPCHK(hipEventElapsedTime(&t, ev[kEvSubmit], tev[ce.end]));
			out->total_ms = std::max(out->total_ms, t);
		}
	HIPCHK(hipEventElapsedTime(&out->windows_ms, tev[kMarkWindows], tev[kMarkWindowsEnd]));
	if (has_tfa2) {
		HIPCHK(hipEventElapsedTime(&out->spec_biquad_ms, tev[kMarkTfa2Spec], tev[kMarkTfa2Repair]));
		HIPCHK(hipEventElapsedTime(&out->repair_biquad_ms, tev[kMarkTfa2Repair], tev[kMarkTfa2Fix]));
		HIPCHK(hipEventElapsedTime(&out->fix_biquad_ms, tev[kMarkTfa2Fix], tev[kMarkTfa2BiquadEnd]));
		HIPCHK(hipEventElapsedTime(&out->slicer_ms, tev[kMarkTfa2Slicer], tev[kMarkTfa2Coop]));
		HIPCHK(hipEventElapsedTime(&out->coop_slicer_ms, tev[kMarkTfa2Coop], tev[kMarkTfa2Decode]));
		HIPCHK(hipEventElapsedTime(&out->decode_ms, tev[kMarkTfa2Decode], tev[kMarkTfa2Commit]));
		HIPCHK(hipEventElapsedTime(&out->commit_ms, tev[kMarkTfa2Commit], tev[kMarkTfa2End]));
	}
	if (has_tfa1) {
		HIPCHK(hipEventElapsedTime(&out->tfa1_slicer_ms, tev[kMarkTfa1Slicer], tev[kMarkTfa1Coop]));
		HIPCHK(hipEventElapsedTime(&out->tfa1_coop_slicer_ms, tev[kMarkTfa1Coop], tev[kMarkTfa1Decode]));
		HIPCHK(hipEventElapsedTime(&out->tfa1_decode_commit_ms, tev[kMarkTfa1Decode], tev[kMarkTfa1End]));
	}
	if (has_whb) {
		HIPCHK(hipEventElapsedTime(&out->whb_biquad_ms, tev[kMarkWhbSpec], tev[kMarkWhbBiquadEnd]));
		HIPCHK(hipEventElapsedTime(&out->whb_demod_ms, tev[kMarkWhbDemod], tev[kMarkWhbDemodEnd]));
		if (hipEventQuery(tev[kMarkWhbCheckEnd]) == hipSuccess &&
		    hipEventElapsedTime(&out->whb_verify_ms, tev[kMarkWhbCheck], tev[kMarkWhbCheckEnd]) != hipSuccess)
			out->whb_verify_ms = 0;
		(void)hipGetLastError();
		// whb_decode_ms / whb_commit_ms stay 0: those stages run in the tail of whb_demod_kernel
	}
	return TFREC_AMD_OK;
}

int tfrec_amd_get_layout(tfrec_amd_ctx *c, int *n_streams)
{
	if (!c || !n_streams)
		return TFREC_AMD_E_INVAL;
	*n_streams = (c->cfg.flags & TFREC_AMD_F_SERIAL_CHAINS) ? 2 : (c->deep ? 6 : 4);
	return TFREC_AMD_OK;
}

int tfrec_amd_get_memory(tfrec_amd_ctx *c, uint64_t *device_bytes, uint64_t *pinned_host_bytes)
{
	if (!c || !device_bytes || !pinned_host_bytes)
		return TFREC_AMD_E_INVAL;
	*device_bytes = c->dev_bytes;
	for (size_t b : c->stage_bytes)  // staging of tfrec_amd_submit_host, grown on demand
		*device_bytes += b;
	*pinned_host_bytes = c->pinned_bytes;
	return TFREC_AMD_OK;
}

int tfrec_amd_get_stats(tfrec_amd_ctx *c, tfrec_amd_stats *out)
{
	if (!c || !out)
		return TFREC_AMD_E_INVAL;
	memset(out, 0, sizeof(*out));
	if (!c->win[0].stats)
		return TFREC_AMD_OK;
	TRY(tfrec_amd_sync(c));
	constexpr int kCounters = (int)(sizeof(tfrec_amd_stats) / sizeof(uint64_t));
	static_assert(sizeof(tfrec_amd_stats) == 11 * sizeof(uint64_t) && kCounters <= 16, "the counters are the first slots of WinTables::stats");
	for (int k = 0; k < kSets; k++) {  // the table sets count separately
		tfrec_amd_stats part;
		HIPCHK(hipMemcpy(&part, c->win[k].stats, sizeof(part), hipMemcpyDeviceToHost));
		for (int i = 0; i < kCounters; i++)
			reinterpret_cast<uint64_t *>(out)[i] += reinterpret_cast<const uint64_t *>(&part)[i];
	}
	return TFREC_AMD_OK;
}
