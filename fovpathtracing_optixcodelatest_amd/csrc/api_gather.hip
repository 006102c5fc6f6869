// api_gather.hip -- multi-GPU over the C ABI: the packed gather of the owned pixels (plan, pack, unpack) and its transport.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <dlfcn.h>

#include "fovpt_ctx.h"

// ---- multi-GPU: the transport between pack and unpack, RCCL over xGMI, for C / C++ hosts ----------------------------
// One process (or thread) per GPU, each with its own fovpt_ctx; the gather of a frame is
//   plan -> pack (HIP) -> ncclGroupStart; ncclSend to the root; on the root ncclRecv from every rank; ncclGroupEnd -> unpack
// all enqueued on fovpt_stream(), the stream frames complete on: no host synchronisation, and the transport of frame k runs
// beside the rendering of frame k + 1.  librccl is loaded at run time so that libfovpt.so has no link-time dependency on it
// (a process that already holds an RCCL -- PyTorch's -- gets that one: same SONAME).
namespace {
struct Rccl {
    void* lib = nullptr;
    bool tried = false;
    std::string why;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
Rccl& rccl()
{
    static Rccl R;
    if (R.tried) return R;
    R.tried = true;
    // A copy the process already holds comes first (RTLD_NOLOAD): a host that has PyTorch loaded has PyTorch's bundled
    // librccl.so -- another file than /opt/rocm's librccl.so.1, so asking for the latter by name would put a SECOND RCCL into the
    // process (fovpathtracing_optixcodelatest_amd/lib.py loads torch's copy first when torch is installed and not imported yet).
    const char* names[] = {getenv("FOVPT_RCCL_LIB"), "librccl.so", "librccl.so.1", "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (int k = 0; k < 6 && !R.lib; k++) {
        const char* n = names[k];
        if (!n || !*n) continue;
        const bool only_if_loaded = k == 1 || k == 2;
        // (RTLD_LOCAL: every entry point is looked up with dlsym, and RCCL brings librocm_smi64 with it, whose `amd::smi` globals
        // must not become the process's: /opt/rocm's libamd_smi.so -- which PyTorch's device queries load -- defines the same ones,
        // and two libraries then run their static destructors on one object)
        R.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL | (only_if_loaded ? RTLD_NOLOAD : 0));
        // (dlerror() clears the message it returns: a second call gives NULL)
        if (!R.lib && !only_if_loaded) { const char* e = dlerror(); R.why = e ? e : "dlopen failed"; }
    }
    if (!R.lib) { if (R.why.empty()) R.why = "librccl not found"; return R; }
    struct { const char* n; void** f; } syms[] = {
        {"ncclGetUniqueId", (void**)&R.GetUniqueId}, {"ncclCommInitRank", (void**)&R.CommInitRank}, {"ncclCommDestroy", (void**)&R.CommDestroy},
        {"ncclGroupStart", (void**)&R.GroupStart}, {"ncclGroupEnd", (void**)&R.GroupEnd}, {"ncclSend", (void**)&R.Send}, {"ncclRecv", (void**)&R.Recv},
        {"ncclGetErrorString", (void**)&R.GetErrorString}};
    for (auto& sy : syms) {
        *sy.f = dlsym(R.lib, sy.n);
        if (!*sy.f) { R.why = std::string("librccl lacks ") + sy.n; dlclose(R.lib); R.lib = nullptr; return R; }
    }
    return R;
}
#define NCCLCHK(c, x) do { ncclResult_t r_ = (x); if (r_ != ncclSuccess) return fail((c), FOVPT_E_DEVICE, "%s: %s", #x, rccl().GetErrorString(r_)); } while (0)
}  // namespace

extern "C" {

// ---- multi-GPU: packed gather of the owned pixels ---------------------------------------------------
int fovpt_gather_plan(fovpt_ctx* c, const fovpt_launch_params* lp, uint32_t* counts_out, int counts_len)
{
    if (!c || !lp) return FOVPT_E_INVALID;
    const int world = c->cfg.world < 1 ? 1 : c->cfg.world;
    if (world > 64) return fail(c, FOVPT_E_INVALID, "gather plans support up to 64 ranks (world = %d)", world);
    if (lp->frame.size.x <= 0 || lp->frame.size.y <= 0) return fail(c, FOVPT_E_INVALID, "bad frame size");
    if (counts_out && counts_len < world) return fail(c, FOVPT_E_INVALID, "counts_out holds %d entries, world is %d", counts_len, world);
    HIPCHK(c, hipSetDevice(c->device));
    char key[256];
    snprintf(key, sizeof(key), "%d x %d u%d r%d/%d c%u,%u w%d t%dx%d", lp->frame.size.x, lp->frame.size.y, c->cfg.uniform, c->cfg.r_inner, c->cfg.r_outer,
             lp->frame.c.x, lp->frame.c.y, world, c->cfg.tile_w, c->cfg.tile_h);
    if (c->plan_key != key) {
        FrameDev fd;
        frame_levels(c->cfg, lp, fd);
        fd.rank = c->cfg.rank; fd.world = world;
        fd.tile_w = c->cfg.tile_w > 0 ? c->cfg.tile_w : 8; fd.tile_h = c->cfg.tile_h > 0 ? c->cfg.tile_h : 4;
        const uint32_t npix = (uint32_t)fd.w * (uint32_t)fd.h, nblocks = (npix + FOVPT_BLOCK - 1) / FOVPT_BLOCK;
        HIPCHK(c, c->plan_owner.reserve(npix));
        HIPCHK(c, c->plan_blocks.reserve((size_t)nblocks * world * 4));
        HIPCHK(c, c->plan_total.reserve(64 * 4));
        HIPCHK(c, c->plan_base.reserve(65 * 4));
        HIPCHK(c, c->plan_idx.reserve((size_t)npix * 4));
        hipStream_t st = c->shadow_stream;                  // the stream frames complete on: pack / unpack run there too
        fovpt_launch_plan_owner(st, fd, (uint8_t*)c->plan_owner.p, (uint32_t*)c->plan_blocks.p, nblocks);
        fovpt_launch_plan_scan_fill(st, npix, nblocks, world, (const uint8_t*)c->plan_owner.p, (uint32_t*)c->plan_blocks.p,
                                    (uint32_t*)c->plan_total.p, nullptr, nullptr, 0);
        uint32_t total[64];
        HIPCHK(c, hipMemcpyAsync(total, c->plan_total.p, (size_t)world * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        c->plan_off.assign((size_t)world + 1, 0u);
        for (int r = 0; r < world; r++) c->plan_off[r + 1] = c->plan_off[r] + total[r];
        HIPCHK(c, hipMemcpyAsync(c->plan_base.p, c->plan_off.data(), (size_t)(world + 1) * 4, hipMemcpyHostToDevice, st));
        fovpt_launch_plan_scan_fill(st, npix, nblocks, world, (const uint8_t*)c->plan_owner.p, (uint32_t*)c->plan_blocks.p,
                                    nullptr, (const uint32_t*)c->plan_base.p, (uint32_t*)c->plan_idx.p, 1);
        HIPCHK(c, hipStreamSynchronize(st));                // (plan_off.data() must outlive the copy)
        HIPCHK(c, hipGetLastError());
        c->plan_key = key;
    }
    if (counts_out) for (int r = 0; r < world; r++) counts_out[r] = c->plan_off[r + 1] - c->plan_off[r];
    return FOVPT_OK;
}

int fovpt_gather_pack(fovpt_ctx* c, const uint32_t* frame, uint32_t* packed)
{
    if (!c || !frame || !packed) return FOVPT_E_INVALID;
    if (c->plan_key.empty()) return fail(c, FOVPT_E_INVALID, "fovpt_gather_pack without a plan (fovpt_gather_plan)");
    HIPCHK(c, hipSetDevice(c->device));
    const int r = c->cfg.rank;
    if (r < 0 || (size_t)r + 1 >= c->plan_off.size()) return fail(c, FOVPT_E_INVALID, "rank %d is not part of the plan", r);
    fovpt_launch_gather_pack(c->shadow_stream, c->plan_off[r + 1] - c->plan_off[r], (const uint32_t*)c->plan_idx.p + c->plan_off[r], frame, packed);
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

int fovpt_gather_unpack(fovpt_ctx* c, const uint32_t* gathered, uint32_t stride, uint32_t* frame)
{
    if (!c || !gathered || !frame) return FOVPT_E_INVALID;
    if (c->plan_key.empty()) return fail(c, FOVPT_E_INVALID, "fovpt_gather_unpack without a plan (fovpt_gather_plan)");
    HIPCHK(c, hipSetDevice(c->device));
    const int world = (int)c->plan_off.size() - 1;
    for (int r = 0; r < world; r++)
        if (c->plan_off[r + 1] - c->plan_off[r] > stride) return fail(c, FOVPT_E_INVALID, "stride %u is smaller than rank %d's %u pixels", stride, r, c->plan_off[r + 1] - c->plan_off[r]);
    fovpt_launch_gather_unpack(c->shadow_stream, world, stride, c->plan_off[world], (const uint32_t*)c->plan_base.p, (const uint32_t*)c->plan_idx.p, gathered, frame);
    HIPCHK(c, hipGetLastError());
    return FOVPT_OK;
}

int fovpt_comm_get_unique_id(void* id)
{
    if (!id) return fail(nullptr, FOVPT_E_INVALID, "fovpt_comm_get_unique_id: null argument");
    Rccl& R = rccl();
    if (!R.lib) return fail(nullptr, FOVPT_E_DEVICE, "RCCL is not available: %s", R.why.c_str());
    static_assert(FOVPT_COMM_ID_BYTES == sizeof(ncclUniqueId), "unique id size");
    ncclUniqueId u;
    NCCLCHK(nullptr, R.GetUniqueId(&u));
    memcpy(id, &u, sizeof(u));
    return FOVPT_OK;
}

int fovpt_comm_init(fovpt_ctx* c, const void* id, int rank, int world)
{
    if (!c || !id) return FOVPT_E_INVALID;
    if (world < 1 || world > 64 || rank < 0 || rank >= world) return fail(c, FOVPT_E_INVALID, "bad rank %d of %d (1 .. 64 ranks)", rank, world);
    Rccl& R = rccl();
    if (!R.lib) return fail(c, FOVPT_E_DEVICE, "RCCL is not available: %s", R.why.c_str());
    int rc = fovpt_comm_destroy(c);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    NCCLCHK(c, R.CommInitRank(&c->comm, world, u, rank));      // collective: every rank calls it, each on its own device
    c->comm_rank = rank; c->comm_world = world;
    return FOVPT_OK;
}

int fovpt_comm_destroy(fovpt_ctx* c)
{
    if (!c) return FOVPT_E_INVALID;
    if (!c->comm) return FOVPT_OK;
    (void)hipSetDevice(c->device);
    if (c->shadow_stream) (void)hipStreamSynchronize(c->shadow_stream);
    ncclComm_t comm = c->comm;
    c->comm = nullptr; c->comm_world = 0;
    NCCLCHK(c, rccl().CommDestroy(comm));
    return FOVPT_OK;
}

int fovpt_gather_frame(fovpt_ctx* c, const fovpt_launch_params* lp, int root, const uint32_t* frame, uint32_t* full_frame)
{
    if (!c || !lp || !frame) return FOVPT_E_INVALID;
    if (!c->comm) return fail(c, FOVPT_E_INVALID, "fovpt_gather_frame without a communicator (fovpt_comm_init)");
    const int world = c->comm_world, rank = c->comm_rank;
    if (c->cfg.world != world || c->cfg.rank != rank)
        return fail(c, FOVPT_E_INVALID, "the communicator is rank %d of %d, fovpt_config says %d of %d", rank, world, c->cfg.rank, c->cfg.world);
    if (root < 0 || root >= world) return fail(c, FOVPT_E_INVALID, "bad root %d", root);
    if (rank == root && !full_frame) return fail(c, FOVPT_E_INVALID, "the root needs a frame to gather into");
    uint32_t counts[64];
    int rc = fovpt_gather_plan(c, lp, counts, 64);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    uint32_t stride = 0;
    for (int r = 0; r < world; r++) stride = counts[r] > stride ? counts[r] : stride;
    stride = (stride + 63u) & ~63u;
    if (stride == 0) return FOVPT_OK;                               // no launch index writes any pixel
    HIPCHK(c, c->comm_packed.reserve((size_t)stride * 4));
    if (rank == root) HIPCHK(c, c->comm_gathered.reserve((size_t)stride * 4 * world));
    rc = fovpt_gather_pack(c, frame, (uint32_t*)c->comm_packed.p);
    if (rc) return rc;
    Rccl& R = rccl();
    hipStream_t st = c->shadow_stream;
    // A group that was opened is always closed: the first failing call is remembered, the remaining point-to-point calls are
    // skipped, ncclGroupEnd still runs (an open group would leave this rank's later collectives queued for ever and its peers
    // blocked in theirs), and only then does the call fail.
    NCCLCHK(c, R.GroupStart());
    ncclResult_t first_err = ncclSuccess;
    const char* first_what = "";
    if (rank == root)
        for (int r = 0; r < world && first_err == ncclSuccess; r++)
            if (counts[r]) {
                first_err = R.Recv((uint32_t*)c->comm_gathered.p + (size_t)r * stride, counts[r], ncclUint32, r, c->comm, st);
                first_what = "ncclRecv";
            }
    if (counts[rank] && first_err == ncclSuccess) { first_err = R.Send(c->comm_packed.p, counts[rank], ncclUint32, root, c->comm, st); first_what = "ncclSend"; }
    const ncclResult_t end_err = R.GroupEnd();
    if (first_err != ncclSuccess) return fail(c, FOVPT_E_DEVICE, "%s: %s", first_what, R.GetErrorString(first_err));
    if (end_err != ncclSuccess) return fail(c, FOVPT_E_DEVICE, "ncclGroupEnd: %s", R.GetErrorString(end_err));
    if (rank == root) {
        rc = fovpt_gather_unpack(c, (const uint32_t*)c->comm_gathered.p, stride, full_frame);
        if (rc) return rc;
    }
    return FOVPT_OK;
}

}  // extern "C"
