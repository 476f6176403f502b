// tfrec_amd/csrc/capi_create.h -- tfrec_amd_create step by step, the constructors, destroy: included by capi.hip, which lists what is where.
#pragma once

// ---- biquad coefficients (iir2::set, dsp_stuff.cpp:36-45) in the arithmetic of the reference's normative
// build (oracle/tfrec_oracle.c header).  The five cut-offs the reference ever instantiates
// (main.cpp:186-217, tfa2.cpp:321, whb.cpp:610-611) come from a table of the exact values that build
// produces, so they do not depend on this host's libm tan(); other cut-offs use the formula.
static BiquadCoef biquad_coef(double cutoff)
{
	static const struct {
		double cutoff, b0, a1, a2;
	} known[] = {
		{ 0.5 / (384000.0 / 17240), 0x1.27f98b1037a14p-8, 0x1.cd1527f4a26e2p+0, -0x1.a36a1c41c6995p-1 },
		{ 0.5 / (384000.0 / 9600), 0x1.7ed02b18a270dp-10, 0x1.e397ac010fc89p+0, -0x1.ca2cf85850d62p-1 },
		{ 0.5 / (384000.0 / 8842), 0x1.461fa1a309718p-10, 0x1.e5d4f47377e30p+0, -0x1.ce36282a35d90p-1 },
		{ 2.0 / 64.0, 0x1.14a67102a1ffdp-7, 0x1.b949652fa3970p+0, -0x1.83dd316f714e0p-1 },
		{ 0.0025 / 64.0, 0x1.02ae4cfc8910ap-26, 0x1.ffe9409fe171bp+0, -0x1.ffd283451f7d3p-1 },
	};
	BiquadCoef c;
	for (const auto &k : known)
		if (k.cutoff == cutoff) {
			c.b0 = k.b0;
			c.b1 = k.b0 + k.b0;
			c.b2 = k.b0;
			c.a1 = k.a1;
			c.a2 = k.a2;
			return c;
		}
	const double i = 1.0 / tan(cutoff * M_PI);
	const double s = sqrt(2.0);
	const double b0 = 1.0 / ((i + s) * i + 1.0);
	const double t = i * i - 1.0;
	c.b0 = b0;
	c.b1 = b0 + b0;
	c.b2 = b0;
	c.a1 = (t + t) * b0;
	c.a2 = ((s - i) * i - 1.0) * b0;
	return c;
}

static int d2i_host(double v)
{
	if (!(v > -2147483649.0 && v < 2147483648.0))
		return (int)0x80000000;
	return (int)v;
}

// constructor state of a chain: tfa1.cpp:136-141, tfa2.cpp:316-334, whb.cpp:605-623, decoders :36-45/:54-62/:77-107
static ChainState chain_init_state()
{
	ChainState st;
	memset(&st, 0, sizeof(st));
	st.sr_cnt = -1;
	st.dmin = 32767;
	st.dmax = -32767;
	return st;
}

// A stream's settings as the kernels read them: the active slots (launch order) of its types, its threshold (auto: 500, where
// its FskState starts), its longest window, its taps
// second-stage taps: dsp_stuff.cpp:61-88 (narrow) / :91-117 (wide, -W)
static const int16_t kNarrowTaps[20] = { -1087, -1082, -1065, -451, 912, 2997, 5556, 8157, 10285, 11484,
					 11484, 10285, 8157, 5556, 2997, 912, -451, -1065, -1082, -1087 };
static const int16_t kWideTaps[20] = { 546, 451, -317, -1844, -3198, -2817, 494, 6469, 13074, 17421,
				       17421, 13074, 6469, 494, -2817, -3198, -1844, -317, 451, 546 };

// The resampling stage's tap table (tfrec_amd/resample.py restates it): h[phi][n], phi < q, n < t = 2 ceil(3 p / q).
// With dn = (n - t/2 + 1) q - phi the tap offset is d = dn / q and d / r = dn / p:
//   g = sinc(dn / p) (0.54 + 0.46 cos(2 pi dn / (q t))),  v = g 65536 / sum g,  h = round(v), and the residual 65536 - sum h goes to
//   the tap with the largest v (the lowest n among equals).
// false: the rate is outside 1 < p/q < 10, q <= 64 or q | 1536, gcd = 1, or refused -- a v within 1e-9 of a rounding tie (the table
// must not depend on the host's libm), or max_phi sum |h| * 8192 >> 16 >= 32768 (the int16 store could wrap).
static bool resample_table(int32_t p, int32_t q, std::vector<int32_t> &h, int &t)
{
	if (p <= 0 || q <= 0 || (q > kRsQMax && kRsQDiv % q != 0) || p <= q || (long long)p >= 10LL * q)
		return false;
	for (int a = p, b = q; b;) {  // gcd
		const int r = a % b;
		a = b;
		b = r;
		if (!b && a != 1)
			return false;
	}
	t = 2 * ((3 * p + q - 1) / q);  // (p < 10 * 1536)
	h.assign((size_t)q * (size_t)t, 0);
	std::vector<double> v((size_t)t);
	for (int phi = 0; phi < q; phi++) {
		double total = 0.0;
		for (int n = 0; n < t; n++) {
			const double dn = (double)((n - t / 2 + 1) * q - phi);
			const double u = M_PI * dn / p;
			v[n] = (dn == 0.0 ? 1.0 : sin(u) / u) * (0.54 + 0.46 * cos(2.0 * M_PI * dn / ((double)q * t)));
			total += v[n];
		}
		long long sum = 0, sum_abs = 0;
		int best = 0;
		for (int n = 0; n < t; n++) {
			v[n] = v[n] * 65536.0 / total;
			if (fabs(fabs(v[n] - floor(v[n])) - 0.5) < 1e-9)
				return false;
			const int32_t r = (int32_t)floor(v[n] + 0.5);
			h[(size_t)phi * t + n] = r;
			sum += r;
			if (v[n] > v[best])
				best = n;
		}
		h[(size_t)phi * t + best] += (int32_t)(65536 - sum);
		for (int n = 0; n < t; n++)
			sum_abs += llabs((long long)h[(size_t)phi * t + n]);
		if (((sum_abs * 8192) >> 16) >= 32768)
			return false;
	}
	return true;
}

static StreamCfg device_cfg(const tfrec_amd_ctx *c, const tfrec_amd_stream_config &sc)
{
	StreamCfg d;
	memset(&d, 0, sizeof(d));
	for (int a = 0; a < c->launch.n_active; a++)
		if (sc.types_mask & (1 << c->launch.params[a].sensor_type)) {
			d.amask |= 1u << a;
			d.wmax = std::max(d.wmax, (int32_t)c->launch.params[a].window);
		}
	d.thresh = thresh_or_auto(sc.thresh);
	d.autoth = sc.thresh == 0;
	d.wide = (uint16_t)sc.filter_type;
	return d;
}

// ================================================================================ tfrec_amd_create, step by step
static int validate(const tfrec_amd_config *cfg)
{
	if (cfg->n_streams < 1 || cfg->n_streams > 65535 || cfg->max_blocks < 1 || cfg->max_blocks > 4096 ||
	    cfg->max_events < 1 || (cfg->types_mask & 0x2f) == 0 || (cfg->types_mask & ~0x2f) != 0 ||
	    cfg->filter_type < 0 || cfg->filter_type > 1) {
		snprintf(g_err, sizeof(g_err), "bad config");
		return TFREC_AMD_E_INVAL;
	}
	if (cfg->thresh < 0) {
		snprintf(g_err, sizeof(g_err), "thresh must be >= 0 (0 = the reference's auto mode)");
		return TFREC_AMD_E_INVAL;
	}
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
		snprintf(g_err, sizeof(g_err), "no HIP device available");
		return TFREC_AMD_E_HIP;
	}
	if (cfg->device < 0 || cfg->device >= ndev)
		return TFREC_AMD_E_INVAL;
	return TFREC_AMD_OK;
}

// the parameters of a chain of protocol kind `kind` (0 TFA_1, 1 TFA_2 family, 2 WHB) at `baud`
static int chain_params(ChainParams &p, int kind, double baud)
{
	if (kind == 0) {
		p.window = 400;  // 40*BITPERIOD, tfa1.cpp:34, 148
		p.spb = 10;
		return TFREC_AMD_OK;
	}
	p.spb = (1536000 / 4.0) / baud;
	if (kind == 1) {
		p.window = d2i_host(16 * p.spb);  // tfa2.cpp:355
		// multiplier form of numbits (ChainParams::nb_mul), accepted only if it reproduces the fp64 expression
		// for every argument the slicer can form
		const int hmax = (int)(16 * p.spb) + 2;
		const uint64_t a0 = (uint64_t)((double)(1ull << 40) / p.spb);
		for (uint64_t a_try : { a0, a0 + 1, a0 - 1 }) {
			bool ok = true;
			for (int h = 0; h <= hmax && ok; h++)
				ok = tfa2_numbits_mul(2 * h, a_try) == (int)(((double)h + p.spb / 2) / p.spb);
			if (ok) {
				p.nb_mul = a_try;
				break;
			}
		}
		p.td_lo = (int)floor(p.spb / 4) + 1;
		p.td_hi = (int)ceil(32 * p.spb) - 1;
		p.iir = biquad_coef(0.5 / p.spb);  // tfa2.cpp:321
		return TFREC_AMD_OK;
	}
	// whb_demod_kernel's candidate walk has the reference's 64 samples per bit (main.cpp:217) built in (chains2.hip: kWhbSpb)
	if (p.spb != 64.0) {
		snprintf(g_err, sizeof(g_err), "WHB chain with %.3f samples per bit: only 64 is built", p.spb);
		return TFREC_AMD_E_INVAL;
	}
	p.window = d2i_host(8 * p.spb);         // whb.cpp:641
	p.iir = biquad_coef(2.0 / p.spb);       // whb.cpp:610
	p.iir_avg = biquad_coef(0.0025 / p.spb); // whb.cpp:611
	return TFREC_AMD_OK;
}

// the chains of cfg->types_mask in registration order (types and samples-per-bit of main.cpp:173-218), their state arrays
static int register_chains(tfrec_amd_ctx *c)
{
	static const struct {
		int sensor_type, kind, min_bytes;
		double baud;
	} reg[kNSlots] = { { 0, 0, 10, 0 }, { 1, 1, 7, 17240 }, { 2, 1, 7, 9600 }, { 3, 1, 7, 8842 }, { 5, 2, 11, 6000 } };
	const size_t n = (size_t)c->cfg.n_streams;
	const std::vector<ChainState> init(n, chain_init_state());
	for (int s = 0; s < kNSlots; s++) {
		if (!(c->cfg.types_mask & (1 << reg[s].sensor_type)))
			continue;
		const int a = c->launch.n_active++;
		c->launch.slot[a] = s;
		ChainParams &p = c->launch.params[a];
		memset(&p, 0, sizeof(p));
		p.kind = reg[s].kind;
		p.sensor_type = reg[s].sensor_type;
		p.min_bytes = reg[s].min_bytes;
		TRY(chain_params(p, p.kind, reg[s].baud));
		TRY(own_device(c, c->launch.states[a], n * sizeof(ChainState)));
		HIPCHK(hipMemcpy(c->launch.states[a], init.data(), n * sizeof(ChainState), hipMemcpyHostToDevice));
		c->wmax = std::max(c->wmax, (int)p.window);
	}
	return TFREC_AMD_OK;
}

// a carried history's buffers, as a start leaves them
static int make_history(tfrec_amd_ctx *c, Carried &h, int n_bufs)
{
	const size_t bytes = (size_t)c->cfg.n_streams * (size_t)h.bytes;
	for (int k = 0; h.bytes && k < n_bufs; k++) {
		TRY(own_device(c, h.buf[k], bytes));
		HIPCHK(hipMemset(h.buf[k], h.fill, bytes));
	}
	return TFREC_AMD_OK;
}

// the resampling stage's tap table on the device, and rate_abs
static int make_rate_table(tfrec_amd_ctx *c)
{
	InputPath &I = c->input;
	std::vector<int32_t> h;
	int t = 0;
	if (!resample_table(I.rate.p, I.rate.q, h, t))  // (tfrec_amd_create_rate checked it already)
		return TFREC_AMD_E_INVAL;
	I.rate.t = t;
	for (int phi = 0; phi < I.rate.q; phi++) {
		long long a = 0;
		for (int k = 0; k < t; k++)
			a += llabs((long long)h[(size_t)phi * t + k]);
		I.rate_abs = std::max(I.rate_abs, a);
	}
	std::vector<float> hf(h.size());
	if (rs_streamed(I.rate.q, t)) {  // resample_stream_kernel's table: [t][q], h / 65536, column j the phase (j P) mod Q
		const size_t q = (size_t)I.rate.q;
		for (size_t j = 0; j < q; j++) {
			const size_t phi = j * (size_t)I.rate.p % q;
			for (size_t k = 0; k < (size_t)t; k++)
				hf[k * q + j] = (float)h[phi * t + k] * (1.0f / 65536.0f);  // exact: |h| < 2^17
		}
	} else {
		for (size_t i = 0; i < h.size(); i++)
			hf[i] = (float)h[i] * (1.0f / 1024.0f);  // exact: |h| < 2^17
	}
	float *d_taps = nullptr;
	TRY(own_device(c, d_taps, hf.size() * sizeof(float)));
	HIPCHK(hipMemcpy(d_taps, hf.data(), hf.size() * sizeof(float), hipMemcpyHostToDevice));
	I.rate.taps = d_taps;
	return TFREC_AMD_OK;
}

// the front end: its taps, outputs (one set per submit in flight), the auto threshold, and the input path's buffers: the two
// carried histories (here their bytes and fills are decided, once), stage 0 and the rate's tap table
static int make_front_buffers(tfrec_amd_ctx *c)
{
	const tfrec_amd_config &cfg = c->cfg;
	InputPath &I = c->input;
	const size_t m_max = (size_t)cfg.max_blocks * kBlockDec;
	const size_t n = (size_t)cfg.n_streams;
	// second-stage taps (kNarrowTaps / kWideTaps), as h / 65536
	for (int k = 0; k < 20; k++) {
		c->taps.f2[k][0] = c->taps.f2[k][1] = (float)(cfg.filter_type ? kWideTaps[k] : kNarrowTaps[k]) / 65536.0f;
		c->taps.w[k][0] = c->taps.w[k][1] = (float)kWideTaps[k] / 65536.0f;
	}
	c->taps.scfg = nullptr;
	c->dec_stride = m_max;
	c->mask_stride = m_max / 64;
	for (int k = 0; k < kSets; k++) {
		TRY(own_device(c, c->d_dec[k], n * c->dec_stride * sizeof(uint32_t) + 256));  // + slack: K3 loads whole 32-sample chunks at window tails
		TRY(own_device(c, c->d_mask[k], n * c->mask_stride * sizeof(unsigned long long)));
	}
	// every stream starts with the context's threshold (auto: 500)
	TRY(own_device(c, c->d_fsk, n * sizeof(FskState)));
	const std::vector<FskState> fsk(n, FskState{ thresh_or_auto(cfg.thresh), 0, 0, -(1 << 28) });
	HIPCHK(hipMemcpy(c->d_fsk, fsk.data(), n * sizeof(FskState), hipMemcpyHostToDevice));
	for (int k = 0; k < kSets; k++) {
		TRY(own_device(c, c->d_fmdev[k], n * m_max * sizeof(int16_t) + 256));  // + slack: K3 reads whole dwords past an odd tail
		TRY(own_device(c, c->d_prevdec[k], n * sizeof(uint32_t)));
	}
	if (I.channel()) {  // no FIR, the carried state is every stream's last pair ((0, 0) at the start)
		TRY(own_device(c, c->decin.d_last, n * sizeof(uint32_t)));
		HIPCHK(hipMemset(c->decin.d_last, 0, n * sizeof(uint32_t)));
	}
	// zero FIR history == u8 value 128 (decimate::decimate zeroes hist0, dsp_stuff.cpp:145-152); behind a pre-stage the history
	// is int16, twice as wide, and zero
	I.tail.bytes = I.in16() ? 2 * kTailBytes : kTailBytes;
	I.tail.fill = I.in16() ? 0 : 0x80;
	TRY(make_history(c, I.tail, 2));
	if (I.in16()) {
		I.in16_stride = 4 * m_max;  // complex samples at 1.536 MS/s per stream and submit
		for (int k = 0; k < kSets; k++)
			TRY(own_device(c, I.d_in16[k], n * I.in16_stride * sizeof(uint32_t)));
	}
	// the pre-stage's history: raw u8 (silence is 128) or, a rate context reading another format, x (silence is 0)
	const bool raw = I.pre_fmt == TFREC_AMD_FMT_U8;
	switch (I.kind) {
	case PreStage::kDecim10:
		I.pre.bytes = k10xTail;
		I.pre.fill = 0x80;
		TRY(make_history(c, I.pre, kSets));  // (one per set, two used: see Carried)
		break;
	case PreStage::kResample:
		I.pre.bytes = raw ? kRateTail : kFmtTail;
		I.pre.fill = raw ? 0x80 : 0;
		TRY(make_history(c, I.pre, 2));
		TRY(make_rate_table(c));
		break;
	case PreStage::kNone:
	case PreStage::kIngest:
	case PreStage::kChannel:
		break;
	}
	return TFREC_AMD_OK;
}

// One estimator's carried state (a row before its first submit: no window, m = head = 0) and every set's table
template <class Ring>
static int make_estimator(tfrec_amd_ctx *c, Estimator<Ring> &e)
{
	if (!e.k)
		return TFREC_AMD_OK;
	const InputCorrection &o = c->fix;
	const size_t rows = (size_t)o.rows;
	TRY(own_device(c, e.d_ring, rows * (size_t)e.k * sizeof(Ring)));
	TRY(own_device(c, e.d_state, rows * sizeof(int2)));
	HIPCHK(hipMemset(e.d_state, 0, rows * sizeof(int2)));
	for (int k = 0; k < kSets; k++)
		TRY(own_device(c, e.d_table[k], rows * (size_t)o.win_stride * sizeof(uint32_t)));
	e.reset_marked.assign(rows, 0);
	return TFREC_AMD_OK;
}

// tfrec_amd_create_dc / tfrec_amd_create_iq: the estimators, a submit's sums and moments, and every set's corrected rows
static int make_correct(tfrec_amd_ctx *c)
{
	InputCorrection &o = c->fix;
	if (!o.on())
		return TFREC_AMD_OK;
	// the largest submit: floor(max_blocks * 32768 * P / Q) complex samples per row, up to a whole chunk; its whole windows
	const long long n_max = ((long long)c->cfg.max_blocks * (TFREC_AMD_BLOCK_BYTES / 2) * c->input.rate.p / c->input.rate.q + 7) & ~7LL;
	const size_t wins = (size_t)o.rows * (size_t)(n_max / 512);
	o.win_stride = (int)(n_max / 512);
	o.x_stride = (size_t)n_max * 4;
	TRY(make_estimator(c, o.dc));
	TRY(make_estimator(c, o.iq));
	if (o.dc.k)  // (behind the balancer its five sums are used and these are not: kept, tfrec_amd_get_memory reports them)
		TRY(own_device(c, o.d_dc_sums, wins * sizeof(int2)));
	if (o.iq.k) {
		TRY(own_device(c, o.d_iq_sums, wins * sizeof(IqSums)));
		TRY(own_device(c, o.d_mom, wins * sizeof(IqMoments)));
	}
	for (int k = 0; k < kSets; k++)
		TRY(own_device(c, o.d_x[k], (size_t)o.rows * o.x_stride));
	return TFREC_AMD_OK;
}

// One set's window tables (chains2.hip): the rows and counters of every chain carved out of one block
static int make_win_tables(tfrec_amd_ctx *c, int set)
{
	const size_t m_max = (size_t)c->cfg.max_blocks * kBlockDec;
	const size_t n = (size_t)c->cfg.n_streams;
	const size_t chains = (size_t)c->launch.n_active * n;
	const bool whb = has_kind(c->launch, 2);
	WinTables &T = c->win[set];
	T.cap = (int32_t)(m_max / 356 + 2);  // windows of one chain are > W-1 >= 355 samples apart
	T.slots = (int32_t)(m_max / 32 + (size_t)T.cap + 2);  // window-relative 32-sample slots per chain row
	if ((size_t)T.slots > (size_t)kWhbRecOffMask) {  // WhbStepRec::meta packs a slot index into kWhbRecOffMask's bits
		snprintf(g_err, sizeof(g_err), "max_blocks too large for the WHB step records");
		return TFREC_AMD_E_INVAL;
	}
	// rows only for the chains that use them: ld16 for the TFA_2 family (its slots are adjacent in registration order),
	// checkpoints for the chains with a biquad stage (all but TFA_1, which is registered first)
	int a_ld0 = -1, n_ld = 0, a_ck0 = -1;
	for (int a = 0; a < c->launch.n_active; a++) {
		if (c->launch.params[a].kind == 1) {
			if (a_ld0 < 0)
				a_ld0 = a;
			n_ld = a - a_ld0 + 1;
		}
		if (c->launch.params[a].kind != 0 && a_ck0 < 0)
			a_ck0 = a;
	}
	T.ld_c0 = (int32_t)((a_ld0 < 0 ? 0 : a_ld0) * n);
	T.ck_c0 = (int32_t)((a_ck0 < 0 ? 0 : a_ck0) * n);
	const size_t ck_chains = a_ck0 < 0 ? 0 : chains - (size_t)a_ck0 * n;
	TRY(own_device(c, c->d_ld16[set], std::max<size_t>(1, (size_t)n_ld * n) * (size_t)T.slots * 32 * sizeof(int16_t)));
	if (whb)  // + slack: whb_demod_kernel keeps three 64-sample steps in flight past a row's last window (whb_demod.h)
		TRY(own_device(c, c->d_dev32[set], n * (size_t)T.slots * 32 * sizeof(int32_t) + 4096));
	T.bit_words = (int32_t)(m_max / 64 + 3 * (size_t)T.cap + 8);
	const size_t wins = chains * (size_t)T.cap;
	T.segcap = (int32_t)((m_max / 32 + (size_t)T.cap) / kSegSlots + 2);
	const size_t segs = chains * (size_t)T.segcap;
	T.whbrec_stride = (int32_t)(m_max / 64 + 2 * (size_t)T.cap + 2 + kWhbRecSlack);
	T.whbdense_stride = (int32_t)(m_max + 64);
	T.whbx_stride = (int32_t)(m_max / 64 + 2);
	const size_t nw = whb ? n : 0;  // rows of the WHB arrays
	// The arrays of one block in this order, `count` elements each and rounded up to 256 bytes: laid out once without a base
	// for the block's size, once more on the block
	auto layout = [&](uintptr_t base) {
		size_t off = 0;
		auto carve = [&](size_t count, auto *&...p) {
			((p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + off), off += (count * sizeof(*p) + 255) & ~(size_t)255), ...);
		};
		carve(chains, T.count, T.cont, T.timeout_next);
		carve(wins, T.open, T.close, T.result, T.decode);
		carve(nw * (size_t)T.cap, T.whbstart);
		carve(chains * (size_t)T.bit_words, T.bits);
		carve(kNQueues * wins + chains, T.items);
		carve(kNQueues + 1, T.queue);
		carve(16, T.stats);
		carve(ck_chains * (size_t)T.slots, T.ckpt);
		carve(segs, T.segstart);
		carve(chains, T.vtotal);
		carve(segs, T.segend1, T.segend2, T.segfix, T.segend3, T.segfix2);
		carve(n * (size_t)T.slots, T.cand, T.mark);
		carve(nw * (size_t)T.whbrec_stride, T.whbrec);
		carve(nw, T.whbfail, T.whbsnap, T.whbx0, T.whbseen, T.whbdense_n);
		carve(nw * (size_t)T.whbx_stride, T.whbxbits, T.whbxsnap);
		carve(nw * (size_t)T.whbdense_stride, T.whbdense);
		return off;
	};
	TRY(own_device(c, c->win_block[set], layout(0)));
	layout(reinterpret_cast<uintptr_t>(c->win_block[set]));
	T.overflow = nullptr;  // lives in the set's event block (kEvOverflowOff): make_event_blocks, reset by every submit
	T.whbgen = c->d_whbgen;
	T.whbX = c->d_whbX;
	T.whbscr = c->d_whbscr;
	T.whbpub = nullptr;
	T.whb_test_perturb = c->whb_test_perturb;
	T.tfa1_vec = TFREC_KNOB_INT("TFA1_VEC", 1, 0, 1) != 0;
	T.tfa2_vec = TFREC_KNOB_INT("TFA2_VEC", 1, 0, 1) != 0;
	T.whb_force_fail = c->whb_force_fail;
	T.whbx = c->d_whbx;
	T.timeout_carry = c->d_tcarry;
	T.prevdec = c->d_prevdec[set];
	HIPCHK(hipMemset(T.queue, 0, (kNQueues + 1) * sizeof(WorkQueue)));
	HIPCHK(hipMemset(T.stats, 0, 128));
	return TFREC_AMD_OK;
}

// the window-parallel pipeline's carried state (the window scan's timeout carry, the WHB check's) and every set's window tables
static int make_window_state(tfrec_amd_ctx *c)
{
	const size_t n = (size_t)c->cfg.n_streams;
	const size_t chains = (size_t)c->launch.n_active * n;
	TRY(own_device(c, c->d_tcarry, chains * 4));
	HIPCHK(hipMemset(c->d_tcarry, 0, chains * 4));
	if (has_kind(c->launch, 2)) {  // iir_avg starts from zero like every iir2 (dsp_stuff.cpp:28-34)
		TRY(own_device(c, c->d_whbx, n * sizeof(WhbExact)));
		TRY(own_device(c, c->d_whbcarry, n * sizeof(int)));
		TRY(own_device(c, c->d_whbgen, n * sizeof(uint32_t)));
		TRY(own_device(c, c->d_whbX, n * sizeof(ChainState)));
		TRY(own_device(c, c->d_whbscr, n * sizeof(ChainState)));
		HIPCHK(hipMemset(c->d_whbgen, 0, n * sizeof(uint32_t)));
		HIPCHK(hipMemset(c->d_whbx, 0, n * sizeof(WhbExact)));
		HIPCHK(hipMemset(c->d_whbcarry, 0, n * sizeof(int)));
		// TEST hooks (results stay exact under both: the check's tolerance and the ambiguity rule widen with D, and a forced
		// failure is only a redo) -- clamped, and never silent: a stray variable changes the redo rate, i.e. the speed
		if (const char *tp = TFREC_KNOB_STR("WHB_TEST_PERTURB"))
			c->whb_test_perturb = std::max(-1000000, std::min(1000000, atoi(tp)));
		if (const char *ff = TFREC_KNOB_STR("WHB_FORCE_FAIL"))
			c->whb_force_fail = std::max(0, atoi(ff));
#if TFREC_KNOBS_BUILT
		if (c->whb_test_perturb || c->whb_force_fail)
			fprintf(stderr, "tfrec_amd: TEST hook active (TFREC_AMD_WHB_TEST_PERTURB=%d, TFREC_AMD_WHB_FORCE_FAIL=%d): WHB streams are "
					"redone on purpose, results unchanged, throughput lower\n", c->whb_test_perturb, c->whb_force_fail);
#endif
		HIPCHK(whb_chain_lds_optin());  // (a per-device attribute: this context's device is the current one)
	}
	for (int set = 0; set < kSets; set++)
		TRY(make_win_tables(c, set));
	return TFREC_AMD_OK;
}

// One event block per set: [EventBuf | the window tables' overflow flag, 16 B | pad to 256 | events] on the device and a
// page-locked copy (the drain's device-to-host copy of a submit is ONE copy on the stream that sets the batch period: three
// copies were 0.45 ms of it with their gaps); the fresh header every submit starts from
static int make_event_blocks(tfrec_amd_ctx *c)
{
	const size_t block = kEvHeader + (size_t)c->cfg.max_events * sizeof(tfrec_amd_event);
	EventBuf eb;
	memset(&eb, 0, sizeof(eb));
	eb.capacity = (uint32_t)c->cfg.max_events;
	for (int k = 0; k < kSets; k++) {
		TRY(own_device(c, c->d_evblock[k], block));
		c->d_eb[k] = (EventBuf *)c->d_evblock[k];
		c->d_events[k] = (tfrec_amd_event *)(c->d_evblock[k] + kEvHeader);
		if (c->win[k].count)  // (window-parallel pipeline: its overflow flag lives behind the EventBuf)
			c->win[k].overflow = (int32_t *)(c->d_evblock[k] + kEvOverflowOff);
		HIPCHK(hipMemset(c->d_evblock[k], 0, kEvHeader));
		HIPCHK(hipMemcpy(c->d_eb[k], &eb, sizeof(eb), hipMemcpyHostToDevice));
	}
	TRY(own_device(c, c->d_eb_fresh, kEvFreshBytes));
	HIPCHK(hipMemset(c->d_eb_fresh, 0, kEvFreshBytes));
	HIPCHK(hipMemcpy(c->d_eb_fresh, &eb, sizeof(eb), hipMemcpyHostToDevice));
	for (int k = 0; k < kSets; k++) {
		TRY(own_pinned(c, c->h_evblock[k], block));
		HIPCHK(hipHostGetDevicePointer((void **)&c->h_evblock_dev[k], c->h_evblock[k], 0));
		c->h_eb[k] = (EventBuf *)c->h_evblock[k];
		c->h_events[k] = (tfrec_amd_event *)(c->h_evblock[k] + kEvHeader);
	}
	return TFREC_AMD_OK;
}

// a table of n_streams entries that every submit stages: the set's device copy and its page-locked source
template <class T>
static int make_staged(tfrec_amd_ctx *c, T *(&d)[kSets], T *(&h)[kSets])
{
	const size_t bytes = (size_t)c->cfg.n_streams * sizeof(T);
	for (int k = 0; k < kSets; k++)
		TRY(own_device(c, d[k], bytes));
	for (int k = 0; k < kSets; k++)
		TRY(own_pinned(c, h[k], bytes));
	return TFREC_AMD_OK;
}

// tfrec_amd_reset_streams: the constructor state a reset restores, a list of at most n_streams indices per set, nothing marked
static int make_restarts(tfrec_amd_ctx *c)
{
	Restarts &r = c->restart;
	TRY(own_device(c, r.d_chain_init, sizeof(ChainState)));
	const ChainState init = chain_init_state();
	HIPCHK(hipMemcpy(r.d_chain_init, &init, sizeof(init), hipMemcpyHostToDevice));
	TRY(make_staged(c, r.d_list, r.h_list));
	r.marked.assign((size_t)c->cfg.n_streams, 0);
	r.origin.assign((size_t)c->cfg.n_streams, 0);
	return TFREC_AMD_OK;
}

// every stream starts with the context's settings
static int make_stream_settings(tfrec_amd_ctx *c)
{
	const tfrec_amd_config &cfg = c->cfg;
	StreamSettings &o = c->settings;
	const size_t n = (size_t)cfg.n_streams;
	const tfrec_amd_stream_config sc0 = { cfg.types_mask, cfg.thresh, cfg.filter_type, 0 };
	o.scfg_api.assign(n, sc0);
	o.scfg.assign(n, device_cfg(c, sc0));
	o.n_auto = cfg.thresh == 0 ? (int)n : 0;
	TRY(own_device(c, o.d_scfg, n * sizeof(StreamCfg)));
	HIPCHK(hipMemcpy(o.d_scfg, o.scfg.data(), n * sizeof(StreamCfg), hipMemcpyHostToDevice));
	return make_staged(c, o.d_rcfg, o.h_rcfg);
}

// no stream is tuned, every stream reads its own row
static int make_stream_tunes(tfrec_amd_ctx *c)
{
	StreamTunes &o = c->tunes;
	const size_t n = (size_t)c->cfg.n_streams;
	for (Tune *t : { &o.narrow, &o.wide }) {
		t->hz.assign(n, 0);
		t->inc.assign(n, 0u);
	}
	o.row.resize(n);
	for (size_t s = 0; s < n; s++)
		o.row[s] = (int32_t)s;
	TRY(make_staged(c, o.d_tune, o.h_tune));
	return make_staged(c, o.d_chan, o.h_chan);
}

// TFREC_AMD_F_LEVELS: the level meter's state (every stream starts like its FskState), records and lane
static int make_levels(tfrec_amd_ctx *c)
{
	c->lev.lane.on = (c->cfg.flags & TFREC_AMD_F_LEVELS) != 0;
	if (!c->lev.lane.on)
		return TFREC_AMD_OK;
	const size_t n = (size_t)c->cfg.n_streams;
	TRY(own_device(c, c->lev.d_state, n * sizeof(LevelState)));
	const std::vector<LevelState> lev(n, LevelState{ c->settings.scfg[0].thresh, 0, 0, -(1 << 28) });
	HIPCHK(hipMemcpy(c->lev.d_state, lev.data(), n * sizeof(LevelState), hipMemcpyHostToDevice));
	for (int k = 0; k < kSets; k++)
		TRY(own_device(c, c->lev.d_records[k], n * (size_t)c->cfg.max_blocks * sizeof(tfrec_amd_level)));
	return make_side_lane(c, c->lev.lane);
}

// The stream layout: which streams exist, at which priority, and which are aliases -- into S (every set's PipeCtl starts
// from it) and c->cpy.
//   serial (TFREC_AMD_F_SERIAL_CHAINS): fs, cs, and cp for the drain's copies.
//   shallow (TFREC_AMD_DEEP=0): + t1, aux; the biquad stages and the WHB check are aliases (k2 = cs, kw = aux, vx = aux).
//   deep (the default): + k2, kw of their own, fq and ks (discriminator and speculative pass) when a WHB and a TFA_2-family
//     chain are registered, cq for the drain's copies; the window scan runs at the head of kw (ws) and the WHB check on cp
//     (vx).  Stage A of submit k+1 runs beside stage B of submit k.
// Why (measured):
// - HIP multiplexes the streams of one priority onto GPU_MAX_HW_QUEUES hardware queues (default 4), and two streams that
//   share a queue serialise (profiles/ubench/queues.hip).  The runtime keeps one pool of hardware queues PER PRIORITY:
//   fs / cs / aux / t1 are the high-priority streams, and cp (with k2 / kw in the deep layout) has normal priority -- no pool
//   holds more than four streams, whatever GPU_MAX_HW_QUEUES is.
// - Every pipeline stream except the biquad stages runs at high priority.  With the front end at low priority ("fill what
//   the latency-bound chains leave free") its kernel stretched from 3 to 11 ms beside the chains and, with three submits in
//   flight, became the longest stage of all: 13.4 ms per batch instead of 11.7.  (The biquad stages and cp run at normal
//   priority, 0; the discriminator pass, the TFA_2 family's speculative pass and the drain's copies, when they have streams
//   of their own, at low priority.)
// - The window scan at the head of kw, not behind the front end: the front-end stream is the busiest of all (0.3-1.1 ms less
//   on it per batch).
// - The discriminator pass moves from the front-end stream into the pipeline (the head of the TFA_2-family biquad stage, or
//   fq) when a WHB demodulator is registered: then the WHB chain is the longest and the front-end stream the busiest
//   (measured 12.2 -> 11.8 ms per batch; without WHB the TFA_2 chain is the longest and the move costs 7.7 -> 8.5 ms).
// - fq: the discriminator pass on a LOW-priority stream of its own.  It needs the front end only, not the window scan; at the
//   head of k2 it made that stream (discriminator + five biquad kernels) the one that set the batch period: 6.98 -> 6.60 ms
//   per batch over 100 steps (profiles/r04_ab_fmdev_stream.txt).  The low-priority pool's hardware queues are otherwise
//   unused, so the stream shares none (a fifth normal-priority stream would).
// - ks: the speculative biquad pass of the TFA_2 family on a low-priority stream of its own (when the discriminator pass has
//   its stream): it needs nothing of the submit before (chains2.hip K3a), so it runs beside that submit's repair passes and
//   chain walk on k2.  The third stream of the low-priority pool (with fq and cq): no shared hardware queue.
// - cq: the drain's copies must not queue behind the work of younger submits, so they need a hardware queue of their own.
//   On cp they sat between the WHB checks of consecutive submits and waited for ALL chains of their submit: the check of
//   submit k + 1 could not start before the TFA chains of submit k had ended.  6.32 -> 6.21 ms per batch over
//   100 steps (profiles/r04_ab_copy_stream.txt); the low pool's hardware queues hold only this stream and the
//   discriminator's.
// - vx = cp: the WHB check (whb_chain_kernel, whb_check_kernel, the redo) runs where the drain's copies were until they
//   moved to cq.  A stream of its own would be the FIFTH of normal priority in the process (k2, kw, cp and the caller's): it
//   shared a hardware queue with kw, and the 6 ms verification of submit k held up the WHB biquads of submit k + 2.
static int make_streams(tfrec_amd_ctx *c, PipeCtl &S)
{
	int prio_lo = 0, prio_hi = 0;
	(void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
	hipStream_t cp = nullptr;
	TRY(own_stream(c, S.fs, prio_hi));
	TRY(own_stream(c, cp, 0));
	TRY(own_stream(c, S.cs, prio_hi));
	S.ws = S.fs;
	c->cpy = cp;
	if (c->cfg.flags & TFREC_AMD_F_SERIAL_CHAINS)
		return TFREC_AMD_OK;
	TRY(own_stream(c, S.t1, prio_hi));
	TRY(own_stream(c, S.aux, prio_hi));
	const char *dp = TFREC_KNOB_STR("DEEP");
	c->deep = dp ? atoi(dp) != 0 : true;
	c->fmdev_k2 = has_kind(c->launch, 1) && has_kind(c->launch, 2);
	S.k2 = S.cs;
	S.kw = S.aux;
	S.vx = S.aux;
	if (!c->deep)
		return TFREC_AMD_OK;
	TRY(own_stream(c, S.k2, 0));
	TRY(own_stream(c, S.kw, 0));
	S.ws = S.kw;
	if (c->fmdev_k2) {
		TRY(own_stream(c, S.fq, prio_lo));
		TRY(own_stream(c, S.ks, prio_lo));
	}
	TRY(own_stream(c, c->cpy, prio_lo));
	S.vx = cp;
	return TFREC_AMD_OK;
}

// every set's PipeCtl (the layout's streams and the set's events) and the set's other events
static int make_pipes(tfrec_amd_ctx *c, const PipeCtl &S)
{
	const bool serial = (c->cfg.flags & TFREC_AMD_F_SERIAL_CHAINS) != 0;
	const bool timing = (c->cfg.flags & TFREC_AMD_F_TIMING) != 0;
	for (int k = 0; k < kSets; k++) {
		PipeCtl &P = c->pipe[k];
		P = S;
		for (hipEvent_t *e : { &P.done[0], &P.done[1], &P.done[2], &P.ev_win, &P.ev_fork, &P.ev_k2, &P.ev_kw, &P.ev_fm,
				       &P.ev_spec, &c->ev_in[k], &P.ev_front, &c->copied[k] })
			TRY(own_event(c, *e, hipEventDisableTiming));
		if (!serial)
			TRY(own_event(c, P.ev_aux, hipEventDisableTiming));
		if (timing) {
			for (hipEvent_t &e : c->ev[k])
				TRY(own_event(c, e, hipEventDefault));
			if (!serial) {
				for (hipEvent_t &e : c->tev[k])
					TRY(own_event(c, e, hipEventDefault));
				P.tev = c->tev[k];
			}
		}
		P.whb_carry = c->d_whbcarry;
		P.fmdev_wmax = c->fmdev_k2 ? c->wmax : 0;
		P.fm_flag_eps = c->fm_flag_eps;
	}
	return TFREC_AMD_OK;
}

static int init_context(tfrec_amd_ctx *c)
{
	if (const char *fe = TFREC_KNOB_STR("FM_FLAG_EPS"))
		c->fm_flag_eps = std::max(1e-9, atof(fe));
	if (const char *cg = TFREC_KNOB_STR("COPY_GUESS_MIN"))
		c->copy_guess = c->copy_guess_min = (uint32_t)std::max(1, atoi(cg));
	TRY(register_chains(c));
	TRY(make_front_buffers(c));
	TRY(make_correct(c));
	if (!(c->cfg.flags & TFREC_AMD_F_SERIAL_CHAINS))
		TRY(make_window_state(c));
	TRY(make_event_blocks(c));
	TRY(make_restarts(c));
	TRY(make_stream_settings(c));
	TRY(make_stream_tunes(c));
	PipeCtl streams = {};
	TRY(make_streams(c, streams));
	TRY(make_pipes(c, streams));
	TRY(make_levels(c));
	return TFREC_AMD_OK;
}

static void print_host_prof(const tfrec_amd_ctx *c)
{
	if (TFREC_KNOB_STR("HOST_PROF") && c->hp_n)
		fprintf(stderr, "tfrec_amd host time per batch: submit %.0f us, drain: wait %.0f + copy %.0f + sort %.0f us (%ld batches)\n",
			1e6 * c->hp_submit / c->hp_n, 1e6 * c->hp_wait / c->hp_n, 1e6 * c->hp_copy / c->hp_n, 1e6 * c->hp_sort / c->hp_n,
			c->hp_n);
	if (TFREC_KNOB_STR("HOST_PROF") && c->hp_gap_n)
		fprintf(stderr, "tfrec_amd front-end stream: %.3f ms between one submit's front end and the next one's; front-end start -> TFA_1 chain end %.2f ms; front-end start to start %.3f ms (%ld batches)\n",
			c->hp_gap / c->hp_gap_n, c->hp_lat / c->hp_gap_n, c->hp_s2s / c->hp_gap_n, c->hp_gap_n);
}

int tfrec_amd_destroy(tfrec_amd_ctx *c)
{
	if (!c)
		return TFREC_AMD_OK;
	(void)hipSetDevice(c->cfg.device);
	(void)hipDeviceSynchronize();
	print_host_prof(c);
	release_all(c);
	delete c;
	return TFREC_AMD_OK;
}

// What a constructor asks for behind its own argument checks: the format of the input rows and their rate p / q; decimated: the
// channel-rate input (tfrec_amd_create_decimated); dc_k, iq_k != 0: with the DC blocker, the IQ balancer or both over at most `rows`
// input rows (tfrec_amd_create_dc, tfrec_amd_create_iq)
struct InputSpec {
	int32_t fmt = TFREC_AMD_FMT_U8, p = 1, q = 1;
	bool decimated = false;
	int32_t dc_k = 0, iq_k = 0, rows = 0;
};

// The context made for an input.  Its pre-stage follows from the rate and from the format it reads (pre_fmt: S16, the corrected
// rows, behind a correction stage): see PreStage.
static int create_with(const tfrec_amd_config *cfg, const InputSpec &in, tfrec_amd_ctx **out)
{
	TRY(validate(cfg));
	HIPCHK(hipSetDevice(cfg->device));
	tfrec_amd_ctx *c = new (std::nothrow) tfrec_amd_ctx();
	if (!c)
		return TFREC_AMD_E_NOMEM;
	c->cfg = *cfg;
	InputPath &I = c->input;
	I.fmt = in.fmt;
	I.pre_fmt = in.dc_k || in.iq_k ? TFREC_AMD_FMT_S16 : in.fmt;
	c->fix.dc.k = in.dc_k;
	c->fix.iq.k = in.iq_k;
	c->fix.rows = in.rows;
	const bool base = in.p == 1 && in.q == 1, x10 = (cfg->flags & TFREC_AMD_F_INPUT_10X) != 0;  // (x10: the spec is the default one)
	I.rate.p = x10 ? 10 : in.p;
	I.rate.q = x10 ? 1 : in.q;
	I.kind = x10 ? PreStage::kDecim10 : in.decimated ? PreStage::kChannel : !base ? PreStage::kResample
		 : I.pre_fmt != TFREC_AMD_FMT_U8 ? PreStage::kIngest : PreStage::kNone;
	const int rc = init_context(c);
	if (rc != TFREC_AMD_OK) {
		tfrec_amd_destroy(c);
		return rc;
	}
	*out = c;
	return TFREC_AMD_OK;
}

int tfrec_amd_create(const tfrec_amd_config *cfg, tfrec_amd_ctx **out)
{
	if (!cfg || !out)
		return TFREC_AMD_E_INVAL;
	*out = nullptr;
	return create_with(cfg, InputSpec{}, out);
}

int tfrec_amd_resample_taps(int32_t rate_p, int32_t rate_q, int32_t *taps, int cap, int *n_taps_per_phase)
{
	std::vector<int32_t> h;
	int t = 0;
	if (cap < 0 || (cap > 0 && !taps) || !resample_table(rate_p, rate_q, h, t)) {
		snprintf(g_err, sizeof(g_err), "input rate %d/%d: unsupported or refused", (int)rate_p, (int)rate_q);
		return TFREC_AMD_E_INVAL;
	}
	if (n_taps_per_phase)
		*n_taps_per_phase = t;
	if (taps) {
		if ((size_t)cap < h.size())
			return TFREC_AMD_E_INVAL;
		memcpy(taps, h.data(), h.size() * sizeof(int32_t));
	}
	return TFREC_AMD_OK;
}

int tfrec_amd_create_rate(const tfrec_amd_config *cfg, int32_t rate_p, int32_t rate_q, tfrec_amd_ctx **out)
{
	if (!cfg || !out)
		return TFREC_AMD_E_INVAL;
	*out = nullptr;
	if (cfg->flags & TFREC_AMD_F_INPUT_10X) {
		snprintf(g_err, sizeof(g_err), "an input rate and the 15.36 MS/s input flag exclude each other");
		return TFREC_AMD_E_INVAL;
	}
	TRY(tfrec_amd_resample_taps(rate_p, rate_q, nullptr, 0, nullptr));
	return create_with(cfg, InputSpec{ .p = rate_p, .q = rate_q }, out);
}

// What the constructors that take a format share: a known format, no 10:1 stage behind it (what: the stage that refuses the flag, or
// nullptr, the format itself), and a rate the resampling stage takes
static int check_input(const tfrec_amd_config *cfg, int32_t format, int32_t rate_p, int32_t rate_q, const char *what)
{
	if (format < TFREC_AMD_FMT_U8 || format > TFREC_AMD_FMT_F32) {
		snprintf(g_err, sizeof(g_err), "unknown input format %d", (int)format);
		return TFREC_AMD_E_INVAL;
	}
	if (cfg->flags & TFREC_AMD_F_INPUT_10X) {
		if (what)
			snprintf(g_err, sizeof(g_err), "no %s ahead of the 10:1 stage: the 15.36 MS/s input flag is refused", what);
		else
			snprintf(g_err, sizeof(g_err), "the 15.36 MS/s input flag takes u8 input only");
		return TFREC_AMD_E_INVAL;
	}
	if (rate_p != 1 || rate_q != 1)
		TRY(tfrec_amd_resample_taps(rate_p, rate_q, nullptr, 0, nullptr));
	return TFREC_AMD_OK;
}

int tfrec_amd_create_format(const tfrec_amd_config *cfg, int32_t format, int32_t rate_p, int32_t rate_q, tfrec_amd_ctx **out)
{
	if (!cfg || !out)
		return TFREC_AMD_E_INVAL;
	*out = nullptr;
	if (format == TFREC_AMD_FMT_U8)  // exactly the older constructors
		return rate_p == 1 && rate_q == 1 ? tfrec_amd_create(cfg, out) : tfrec_amd_create_rate(cfg, rate_p, rate_q, out);
	TRY(check_input(cfg, format, rate_p, rate_q, nullptr));
	return create_with(cfg, InputSpec{ .fmt = format, .p = rate_p, .q = rate_q }, out);
}

int tfrec_amd_get_input_format(tfrec_amd_ctx *c, int32_t *format)
{
	if (!c || !format)
		return TFREC_AMD_E_INVAL;
	*format = c->input.fmt;
	return TFREC_AMD_OK;
}

int tfrec_amd_get_input_rate(tfrec_amd_ctx *c, int32_t *p, int32_t *q)
{
	if (!c || !p || !q)
		return TFREC_AMD_E_INVAL;
	*p = c->input.rate.p;
	*q = c->input.rate.q;
	return TFREC_AMD_OK;
}
