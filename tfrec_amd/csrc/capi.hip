// tfrec_amd/csrc/capi.hip -- C ABI (include/tfrec_amd.h): context, submit, drain.  No torch types.  One translation unit, cut by
// concern into the capi_*.h headers below (each needs the ones above it); their entry points have C linkage from tfrec_amd.h.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <new>
#include <type_traits>
#include <vector>

#include "crc_table.h"  // the frame check's settings and term table: plain C++
#include "knobs.h"
#include "tfrec_dev.h"
#include "launch.h"  // every launch_* of frontend.hip, chains.hip and chains2.hip, and the records they take (FrontOut, History, ...)
#include "state.h"   // stream_state_kernel and its segment table (save / load)

using namespace tfrec;

#include "capi_ctx.h"      // constants, errors, the records (InputPath, the per-stream tables, ...), tfrec_amd_ctx and what it owns, guards, checks
#include "capi_create.h"   // chain parameters, tap tables, the context's buffers, streams and events; constructors, destroy
#include "capi_probe.h"    // the discriminator's host check, debug statistics; probes, read-backs, timings, memory, counters
#include "capi_submit.h"   // the two kernels, a submit's resets and staging, submit_common, the submits, drain, sync, pending
#include "capi_outputs.h"  // the level meter's, the recorder's, the spectrum's and the occupancy detector's entry points
#include "capi_correct.h"  // the DC blocker's and the IQ balancer's constructors, getters, reads and resets
#include "capi_streams.h"  // reset, configure, the three tunes, map, and their getters
#include "capi_decin.h"    // the channel-rate constructor, the recorder's pre samples, sparse submits
#include "capi_bursts.h"   // the five burst stages (meter, envelope, clock, track, sync): the shared preflight and readers, each enable and read, the track's four modes, its line code and its frame check
#include "capi_state.h"    // a stream's state blob: its header, the inventory table, save and load

extern "C" {

const char *tfrec_amd_version(void) { return "tfrec_amd 0.1 (gfx950)"; }

int tfrec_amd_fifo_depth(void) { return kSets; }

const char *tfrec_amd_strerror(int code)
{
	switch (code) {
	case TFREC_AMD_OK: return "ok";
	case TFREC_AMD_E_INVAL: return "invalid argument or unsupported configuration";
	case TFREC_AMD_E_NOMEM: return "out of memory";
	case TFREC_AMD_E_HIP: return "HIP runtime error";
	case TFREC_AMD_E_OVERFLOW: return "event buffer overflow";
	case TFREC_AMD_E_STATE: return "call sequence error";
	default: return "unknown error";
	}
}

const char *tfrec_amd_last_error(void) { return g_err; }

int tfrec_amd_rssi_db(int slot, int64_t rssi_raw)
{
	if (slot == TFREC_AMD_SLOT_WHB)  // whb.cpp:696 as compiled: 10*log10(rssi*0.00025 + 1)
		return d2i_host(10 * log10((double)rssi_raw * 0.00025 + 1.0));
	// tfa1.cpp:180, tfa2.cpp:434: (int)(10*log10(rssi)) with an int rssi
	return d2i_host(10 * log10((double)(int)rssi_raw));
}

}  // extern "C"
