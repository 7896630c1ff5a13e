// shim.hip -- kernels' entry point + the extern "C" ABI declared in include/mspack_hip.h.
// Host code elsewhere in the library is plain C and reaches HIP only through these functions.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <thread>
#include <chrono>
#include <vector>
#include <algorithm>
#include <array>
#include "wave_common.hpp"
#include "spec_queue.hpp"
#include "fold_common.hpp"
// ---- the LZX decoder: the same role headers compiled under three configurations, each in its own namespace ----
// lzxn: plain LZX (CAB folders, CHM sections).  mspack_decode_lzx (unit decoder + E8 pass), the resolve tasks of mspack_lzx_pipe,
// mspack_lzx_fold; the frame record's layout everywhere in this file.
namespace lzxn {
#include "lzx_kernel.hpp"
#include "lzx_run.hpp"
#include "lzx_run_plain.hpp"
#include "lzx_pipe.hpp"
#include "lzx_pipe_resolve.hpp"
#include "lzx_unit.hpp"
}
// lzxd: LZX DELTA (OAB blocks).  mspack_decode_lzxd (unit decoder + E8 pass).
#define LZX_DELTA 1
namespace lzxd {
#include "lzx_kernel.hpp"
#include "lzx_run.hpp"
#include "lzx_run_delta.hpp"
#include "lzx_unit.hpp"
}
#undef LZX_DELTA
// lzxp: the parse tasks of mspack_lzx_pipe (no match queue, no token queue, an 8-bit main table: lzx_kernel.hpp).
#define LZX_PARSE_ONLY 1
#define LZX_LIT_RING 1024u      /* bytes of literals a parse wave stages in LDS: they leave as whole 16-byte rows (a power of two) */
#define LZX_STAGE_WORDS 768u    /* 3 KiB of a frame's input per pass + the 1 KiB literal ring: the pipe's 10 KiB LDS block (16 waves per CU).
                                   Measured (profiles/round4_ring_variants.txt): 4 KiB stage + 2 KiB ring at 12 waves per CU 3.00 / 5.87 ms
                                   (4096 / 8192 intervals), 2 KiB + 2 KiB at 16 waves 3.06 / 5.92, this 2.89 / 5.58 */
namespace lzxp {
#include "lzx_kernel.hpp"
#include "lzx_pipe.hpp"
#include "lzx_pipe_parse.hpp"
}
#undef LZX_PARSE_ONLY
static_assert(sizeof(lzxp::LzxFrameRec) == sizeof(lzxn::LzxFrameRec), "one record layout");
#include "mszip_kernel.hpp"
#include "qtm_kernel.hpp"
#include "lzss_kernel.hpp"
#include "lzss_ring_kernel.hpp"
#include "crc32_kernel.hpp"
#include "crc32_range_kernel.hpp"
#include "stored_kernel.hpp"
#include "md5_kernel.hpp"
#include "sha_kernel.hpp"
#include "sha512_kernel.hpp"

// ---- everything behind the decoders: one role header each, in this order ----
// entry_kernels.hpp  pick_unit, the work scratch's layout (lzx_scratch), the map kernels, every __global__ entry point
// launch.hpp         g_err / fail / CK, launch<>, the launch-level knobs, launch_kind, launch_crc32, launch_md5, launch_sha1 / _sha256 / _sha512; the device-resident C ABI
// host_plan.hpp      the host path's chunk planner: plan_batch, a pure function of the unit table (no HIP; tests include it alone)
// host_pins.hpp      page-locked host ranges: the registry, the cut copies, a call's own locks (Pins), mspack_hip_pin / _unpin
// host_stage.hpp     the library's own page-locked staging pool (mspack_hip_stage_alloc / _free)
// host_pipeline.hpp  the host-buffer path: DevCtx, the pipeline (plan -> buffers -> issue -> drain), jobs, shards, release
#include "entry_kernels.hpp"
#include "launch.hpp"
#include "host_plan.hpp"
#include "host_pins.hpp"
#include "host_stage.hpp"
#include "host_pipeline.hpp"
