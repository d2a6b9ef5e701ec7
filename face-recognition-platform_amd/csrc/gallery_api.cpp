// The gallery entry points of libfrp.so (include/frp.h): snapshots of unit fp16 rows, their exact float64 copy, single-row
// updates, zero-copy import (reserve / commit), and the one collective of the multi-GPU path, the RCCL all-gather.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types only: the library opens librccl at first use (frp_dist_*)
#include <dlfcn.h>

#include <cstring>

#include "frp.h"
#include "frp_handle.h"

using namespace frp;

namespace {

// librccl, opened at first use (frp_dist_*: the gallery all-gather; a process that never goes multi-GPU does not load it)
struct Rccl {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::string err;
};
Rccl& rccl() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (r.lib) break;
        }
        const char* why = r.lib ? nullptr : dlerror();       // (read once: a second call returns null)
        if (!r.lib) { r.err = std::string("librccl not found: ") + (why ? why : "?"); return; }
        r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(r.lib, "ncclGetUniqueId");
        r.CommInitRank = (decltype(r.CommInitRank))dlsym(r.lib, "ncclCommInitRank");
        r.CommDestroy = (decltype(r.CommDestroy))dlsym(r.lib, "ncclCommDestroy");
        r.AllGather = (decltype(r.AllGather))dlsym(r.lib, "ncclAllGather");
        r.GetErrorString = (decltype(r.GetErrorString))dlsym(r.lib, "ncclGetErrorString");
        if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.AllGather || !r.GetErrorString) r.err = "librccl lacks an expected symbol";
    });
    return r;
}

// `count` host values of `dtype` (FRP_F16 / F32 / F64) as T = float or double: `src` itself where it holds T already, else cast into `tmp`
template <typename T>
int host_values_as(frp_handle* h, const void* src, size_t count, int dtype, std::vector<T>& tmp, const T** out) {
    *out = (const T*)src;
    if (dtype == (sizeof(T) == 4 ? FRP_F32 : FRP_F64)) return FRP_OK;
    tmp.resize(count);
    auto cast = [&](auto* s) { for (size_t i = 0; i < count; ++i) tmp[i] = (T)s[i]; };
    if (dtype == FRP_F32) cast((const float*)src);
    else if (dtype == FRP_F64) cast((const double*)src);
    else if (dtype == FRP_F16) cast((const _Float16*)src);
    else return fail(h, FRP_ERR_INVALID, "unknown dtype");
    *out = tmp.data();
    return FRP_OK;
}

// exact compat rows: `n` host rows of 512 values of `dtype` -> float64 at dst (device row pointer)
int upload_rows_exact(frp_handle* h, const void* emb, int64_t n, int dtype, double* dst) {
    if (n <= 0) return FRP_OK;
    const size_t cnt = (size_t)n * FRP_EMB_DIM;
    std::vector<double> tmp;
    const double* src;
    FRPCHK(host_values_as(h, emb, cnt, dtype, tmp, &src));
    HIPCHK(h, hipMemcpyAsync(dst, src, cnt * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));      // (tmp / the caller's rows go away)
    return FRP_OK;
}

// a fresh exact matrix with room for `cap_rows` rows, its first `n` widened from unit fp16 device rows (rows installed from device
// data, or that existed before the exact copy was asked for)
int exact_from_f16(frp_handle* h, const void* dev_f16, int64_t n, size_t cap_rows, ScopedBuf& fresh) {
    if (n <= 0) return FRP_OK;
    FRPCHK(ensure(h, fresh, cap_rows * FRP_EMB_DIM * 8));
    hipError_t e = launch_gallery_widen((const _Float16*)dev_f16, (double*)fresh->p, n, FRP_EMB_DIM, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("gallery_widen: ") + hipGetErrorString(e));
    return FRP_OK;
}

// The one place that swaps the snapshot in: `rows` (unit fp16) and `exact` (float64, or empty) become the gallery of `n` rows.  The
// caller has waited for the stream: nothing of this handle still reads the old snapshot.
void install_gallery(frp_handle* h, DevBuf rows, DevBuf exact, int64_t n) {
    release(h->gallery);
    h->gallery = rows;
    release(h->gx);
    h->gx = exact;
    h->g_rows = n;
    h->g_groups.assign((size_t)n, FRP_GROUPS_ALL);      // rows that arrive without a mask are members of every group
    h->g_groups_dev_ok = false;
}

// Rows [first, first + n) of the host mask table have changed (n may reach one past g_rows: the slot a removed last row left, which
// holds 0 on the device): the device copy follows where it exists and has room, else the next grouped match rebuilds it.
int push_groups(frp_handle* h, int64_t first, int64_t n) {
    if (!h->g_groups_dev_ok || n <= 0) return FRP_OK;
    if ((size_t)(first + n) * 4 > h->g_groups_dev.cap) { h->g_groups_dev_ok = false; return FRP_OK; }
    std::vector<uint32_t> v((size_t)n, 0u);
    for (int64_t i = 0; i < n && first + i < h->g_rows; ++i) v[(size_t)i] = h->g_groups[(size_t)(first + i)];
    h->g_groups_dev_ok = false;                          // (a failed copy leaves no half-patched table in use)
    HIPCHK(h, hipMemcpyAsync((uint32_t*)h->g_groups_dev.p + first, v.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->g_groups_dev_ok = true;
    return FRP_OK;
}

// frp_gallery_update_row: `b` (the snapshot or its exact copy) moves to a fresh buffer of `cap_rows` rows that holds its live rows
int grow_rows(frp_handle* h, DevBuf& b, size_t cap_rows, size_t row_bytes, const char* what) {
    ScopedBuf fresh;
    FRPCHK(ensure(h, fresh, cap_rows * row_bytes));
    if (h->g_rows > 0) {
        hipError_t e = hipMemcpyAsync(fresh->p, b.p, (size_t)h->g_rows * row_bytes, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string(what) + hipGetErrorString(e));
    }
    release(b);
    b = fresh.take();
    return FRP_OK;
}

// someone may be writing into a reserved snapshot: until it is committed or cancelled, nothing else replaces or edits the gallery
int refuse_while_reserved(frp_handle* h) {
    return !h->g_reserved.p ? FRP_OK : fail(h, FRP_ERR_INVALID, "a gallery reservation is pending: commit or cancel it first (frp_gallery_commit / frp_gallery_cancel)");
}

}  // namespace

int frp::upload_rows_normalized(frp_handle* h, const float* rows, int64_t n, _Float16* dst) {
    if (n <= 0) return FRP_OK;
    const int64_t chunk = 1 << 16;
    FRPCHK(ensure(h, h->scratch, (size_t)std::min(n, chunk) * FRP_EMB_DIM * 4));
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t m = std::min(chunk, n - r0);
        HIPCHK(h, hipMemcpyAsync(h->scratch.p, rows + r0 * FRP_EMB_DIM, (size_t)m * FRP_EMB_DIM * 4, hipMemcpyHostToDevice, h->stream));
        hipError_t e = launch_gallery_normalize((const float*)h->scratch.p, dst + r0 * FRP_EMB_DIM, m, FRP_EMB_DIM, h->stream);
        if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("gallery_normalize: ") + hipGetErrorString(e));
        HIPCHK(h, hipStreamSynchronize(h->stream));   // scratch is reused by the next chunk
    }
    return FRP_OK;
}

int frp::row_groups_device(frp_handle* h, const uint32_t** out) {
    if (!h->g_groups_dev_ok) {
        // room for the snapshot's row capacity (appends patch in place), a multiple of 32 rows: a wave's block of masks never leaves it
        const size_t cap_rows = std::max<size_t>(h->gallery.cap / ((size_t)FRP_EMB_DIM * 2), (size_t)h->g_rows);
        FRPCHK(ensure(h, h->g_groups_dev, (cap_rows + 31) / 32 * 32 * 4));
        HIPCHK(h, hipMemsetAsync(h->g_groups_dev.p, 0, h->g_groups_dev.cap, h->stream));
        if (h->g_rows > 0)
            HIPCHK(h, hipMemcpyAsync(h->g_groups_dev.p, h->g_groups.data(), (size_t)h->g_rows * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));      // (the table may change as soon as this call returns)
        h->g_groups_dev_ok = true;
    }
    *out = (const uint32_t*)h->g_groups_dev.p;
    return FRP_OK;
}

void frp::dist_shutdown(frp_handle* h) {
    if (!h->comm) return;
    (void)rccl().CommDestroy((ncclComm_t)h->comm);
    h->comm = nullptr;
    h->dist_world = 0;
}

extern "C" {

// ---------------------------------------------------------------- gallery
int frp_gallery_set(frp_handle* h, const void* emb, int64_t n, int32_t d, int32_t dtype) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    h->trk.stale = true;          // (frp.h, face tracks: a cached match must not outlive a change of the rows; set even where the call then fails)
    FRPCHK(refuse_while_reserved(h));
    if (n < 0 || (n > 0 && !emb) || d != FRP_EMB_DIM) return fail(h, FRP_ERR_INVALID, "gallery must be [n x 512]");
    ScopedBuf fresh, fresh_x;   // new snapshot(s), swapped in when complete
    if (n > 0) {
        std::vector<float> f;
        const float* rows;
        FRPCHK(host_values_as(h, emb, (size_t)n * d, dtype, f, &rows));
        FRPCHK(ensure(h, fresh, (size_t)n * d * 2));
        FRPCHK(upload_rows_normalized(h, rows, n, (_Float16*)fresh->p));
        if (h->g_exact) {
            FRPCHK(ensure(h, fresh_x, (size_t)n * d * 8));
            FRPCHK(upload_rows_exact(h, emb, n, dtype, (double*)fresh_x->p));
        }
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    install_gallery(h, fresh.take(), fresh_x.take(), n);
    return FRP_OK;
}

int frp_gallery_set_device(frp_handle* h, const void* dev_f16, int64_t n, int32_t d) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    h->trk.stale = true;          // (frp.h, face tracks: a cached match must not outlive a change of the rows; set even where the call then fails)
    FRPCHK(refuse_while_reserved(h));
    if (n <= 0 || !dev_f16 || d != FRP_EMB_DIM) return fail(h, FRP_ERR_INVALID, "gallery must be [n x 512] fp16 on the device");
    ScopedBuf fresh, fresh_x;
    FRPCHK(ensure(h, fresh, (size_t)n * d * 2));
    hipError_t e = hipMemcpyAsync(fresh->p, dev_f16, (size_t)n * d * 2, hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("gallery copy: ") + hipGetErrorString(e));
    if (h->g_exact) FRPCHK(exact_from_f16(h, fresh->p, n, (size_t)n, fresh_x));
    install_gallery(h, fresh.take(), fresh_x.take(), n);
    return FRP_OK;
}

int frp_gallery_reserve(frp_handle* h, int64_t capacity_rows, void** dev_f16) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!dev_f16 || capacity_rows <= 0 || capacity_rows > 0x7fffff00L) return fail(h, FRP_ERR_INVALID, "bad gallery reservation");
    release(h->g_reserved);
    FRPCHK(ensure(h, h->g_reserved, (size_t)capacity_rows * FRP_EMB_DIM * 2));
    *dev_f16 = h->g_reserved.p;
    return FRP_OK;
}

int frp_gallery_cancel(frp_handle* h) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (h->g_reserved.p) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        release(h->g_reserved);
    }
    return FRP_OK;
}

int frp_gallery_commit(frp_handle* h, int64_t n_rows) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    h->trk.stale = true;          // (frp.h, face tracks: a cached match must not outlive a change of the rows; set even where the call then fails)
    if (!h->g_reserved.p || n_rows < 0 || (size_t)n_rows * FRP_EMB_DIM * 2 > h->g_reserved.cap)
        return fail(h, FRP_ERR_INVALID, "gallery commit without a matching reservation");
    HIPCHK(h, hipStreamSynchronize(h->stream));      // nothing of this handle still reads the old snapshot
    ScopedBuf fresh_x;
    if (h->g_exact) FRPCHK(exact_from_f16(h, h->g_reserved.p, n_rows, (size_t)n_rows, fresh_x));
    install_gallery(h, std::exchange(h->g_reserved, DevBuf()), fresh_x.take(), n_rows);
    return FRP_OK;
}

// ---------------------------------------------------------------- multi-GPU: the one collective of the path, on RCCL
// frames are sharded one stream per GPU and need no exchange; the watch list is the exception - every rank decrypts /
// builds N / R rows and the full unit fp16 matrix is all-gathered over xGMI at load and on updates (the reference holds ENCODINGS
// once, in its one process: backend/app/state.py:78).  The library owns that collective: librccl is opened at first use (dlopen - a
// process that never goes multi-GPU does not load it), the communicator lives in the handle, and the gather lands STRAIGHT in a
// fresh snapshot (shard r at row offset r * ceil(N / R): no compaction copy) that is then installed like any other gallery.
// The caller's launcher (torch.distributed.run, MPI, a shell loop) only has to carry the 128-byte unique id from rank 0 to the others.
static_assert(sizeof(ncclUniqueId) == FRP_DIST_ID_BYTES, "include/frp.h: FRP_DIST_ID_BYTES");

int frp_dist_unique_id(void* id128) {
    if (!id128) return FRP_ERR_INVALID;
    Rccl& r = rccl();
    if (!r.err.empty()) return FRP_ERR_HIP;
    ncclUniqueId id;
    if (r.GetUniqueId(&id) != ncclSuccess) return FRP_ERR_HIP;
    memcpy(id128, &id, sizeof(id));
    return FRP_OK;
}

int frp_dist_init(frp_handle* h, const void* id128, int32_t rank, int32_t world) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!id128 || world <= 0 || rank < 0 || rank >= world) return fail(h, FRP_ERR_INVALID, "bad rank / world size");
    if (h->comm) return fail(h, FRP_ERR_INVALID, "this handle already has a communicator (frp_dist_destroy first)");
    Rccl& r = rccl();
    if (!r.err.empty()) return fail(h, FRP_ERR_HIP, r.err);
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    ncclComm_t c = nullptr;
    const ncclResult_t e = r.CommInitRank(&c, world, id, rank);          // collective over the ranks (the guard has set this handle's device)
    if (e != ncclSuccess) return fail(h, FRP_ERR_HIP, std::string("ncclCommInitRank: ") + r.GetErrorString(e));
    h->comm = c;
    h->dist_rank = rank;
    h->dist_world = world;
    return FRP_OK;
}

int frp_dist_destroy(frp_handle* h) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (h->comm) {
        (void)hipStreamSynchronize(h->stream);
        dist_shutdown(h);
    }
    return FRP_OK;
}

int frp_gallery_allgather(frp_handle* h, const void* shard, int64_t shard_rows, int32_t dtype, int64_t n_total) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    h->trk.stale = true;          // (frp.h, face tracks: a cached match must not outlive a change of the rows; set even where the call then fails)
    if (!h->comm) return fail(h, FRP_ERR_INVALID, "no communicator (frp_dist_init)");
    FRPCHK(refuse_while_reserved(h));
    const int world = h->dist_world, rank = h->dist_rank;
    if (n_total <= 0 || n_total > 0x7fffff00L || shard_rows < 0 || (shard_rows > 0 && !shard)) return fail(h, FRP_ERR_INVALID, "bad shard");
    const int64_t block = (n_total + world - 1) / world;
    const int64_t first = std::min<int64_t>((int64_t)rank * block, n_total), mine = std::min<int64_t>(block, n_total - first);
    if (shard_rows != mine) return fail(h, FRP_ERR_INVALID, "this rank owns rows [rank * ceil(N / R), ...): shard has another row count");
    Rccl& r = rccl();
    // this rank's rows, unit fp16, padded with zero rows to the block size (the last ranks' shards may be short or empty); the gathered
    // blocks never become a reservation of the handle: whatever fails below, they go away with this call
    ScopedBuf send, gathered, fresh_x;
    FRPCHK(ensure(h, send, (size_t)block * FRP_EMB_DIM * 2));
    hipError_t he = hipMemsetAsync(send->p, 0, (size_t)block * FRP_EMB_DIM * 2, h->stream);
    if (he != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("memset: ") + hipGetErrorString(he));
    if (mine > 0) {
        std::vector<float> f;
        const float* rows;
        FRPCHK(host_values_as(h, shard, (size_t)mine * FRP_EMB_DIM, dtype, f, &rows));
        FRPCHK(upload_rows_normalized(h, rows, mine, (_Float16*)send->p));
    }
    FRPCHK(ensure(h, gathered, (size_t)world * block * FRP_EMB_DIM * 2));
    const ncclResult_t e = r.AllGather(send->p, gathered->p, (size_t)block * FRP_EMB_DIM, ncclFloat16, (ncclComm_t)h->comm, h->stream);
    if (e != ncclSuccess) return fail(h, FRP_ERR_HIP, std::string("ncclAllGather: ") + r.GetErrorString(e));
    he = hipStreamSynchronize(h->stream);
    if (he != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("all-gather: ") + hipGetErrorString(he));
    // rows [0, n_total) of the gathered blocks ARE the gallery
    if (h->g_exact) FRPCHK(exact_from_f16(h, gathered->p, n_total, (size_t)n_total, fresh_x));
    install_gallery(h, gathered.take(), fresh_x.take(), n_total);
    return FRP_OK;
}

const void* frp_gallery_device_ptr(frp_handle* h) {
    if (!h) return nullptr;
    Guard g(h);
    return h->g_rows > 0 ? h->gallery.p : nullptr;
}

int frp_gallery_update_row(frp_handle* h, int64_t row, const void* emb, int32_t d, int32_t dtype) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    h->trk.stale = true;          // (frp.h, face tracks: a cached match must not outlive a change of the rows; set even where the call then fails)
    FRPCHK(refuse_while_reserved(h));
    if (!emb || d != FRP_EMB_DIM || row < 0 || row > h->g_rows) return fail(h, FRP_ERR_INVALID, "bad gallery row");
    std::vector<float> f;
    const float* unit;
    FRPCHK(host_values_as(h, emb, (size_t)d, dtype, f, &unit));
    if (row == h->g_rows && (size_t)(h->g_rows + 1) * d * 2 > h->gallery.cap)        // grow: new snapshot with doubled capacity
        FRPCHK(grow_rows(h, h->gallery, (size_t)std::max<int64_t>(1024, h->g_rows * 2), (size_t)d * 2, "gallery grow: "));
    if (h->g_exact && (size_t)(row + 1) * d * 8 > h->gx.cap)        // the exact copy grows with the snapshot's row capacity
        FRPCHK(grow_rows(h, h->gx, std::max<size_t>(h->gallery.cap / ((size_t)d * 2), (size_t)row + 1), (size_t)d * 8, "exact gallery grow: "));
    FRPCHK(upload_rows_normalized(h, unit, 1, (_Float16*)h->gallery.p + row * d));
    if (h->g_exact) FRPCHK(upload_rows_exact(h, emb, 1, dtype, (double*)h->gx.p + row * d));
    if (row == h->g_rows) {          // an append is a member of every group; an overwrite keeps the row's mask
        h->g_groups.push_back(FRP_GROUPS_ALL);
        h->g_rows += 1;
        FRPCHK(push_groups(h, row, 1));
    }
    return FRP_OK;
}

int frp_gallery_remove_row(frp_handle* h, int64_t row) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    h->trk.stale = true;          // (frp.h, face tracks: a cached match must not outlive a change of the rows; set even where the call then fails)
    FRPCHK(refuse_while_reserved(h));
    if (row < 0 || row >= h->g_rows) return fail(h, FRP_ERR_INVALID, "bad gallery row");
    const int64_t last = h->g_rows - 1;
    if (row != last) {
        HIPCHK(h, hipMemcpyAsync((_Float16*)h->gallery.p + row * FRP_EMB_DIM, (_Float16*)h->gallery.p + last * FRP_EMB_DIM,
                                 FRP_EMB_DIM * 2, hipMemcpyDeviceToDevice, h->stream));
        if (h->g_exact)
            HIPCHK(h, hipMemcpyAsync((double*)h->gx.p + row * FRP_EMB_DIM, (double*)h->gx.p + last * FRP_EMB_DIM, FRP_EMB_DIM * 8,
                                     hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    h->g_groups[(size_t)row] = h->g_groups[(size_t)last];      // the mask moves with the row
    h->g_groups.pop_back();
    h->g_rows = last;
    FRPCHK(push_groups(h, row, 1));
    return push_groups(h, last, 1);                            // (rows >= g_rows hold 0 on the device)
}

int64_t frp_gallery_size(const frp_handle* h) { return h ? h->g_rows : -1; }

int frp_gallery_get(frp_handle* h, void* out_f16, int64_t first_row, int64_t n_rows) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!out_f16 || first_row < 0 || n_rows < 0 || first_row + n_rows > h->g_rows) return fail(h, FRP_ERR_INVALID, "bad gallery range");
    if (n_rows == 0) return FRP_OK;
    HIPCHK(h, hipMemcpyAsync(out_f16, (_Float16*)h->gallery.p + first_row * FRP_EMB_DIM, (size_t)n_rows * FRP_EMB_DIM * 2,
                             hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return FRP_OK;
}

int frp_gallery_set_groups(frp_handle* h, const uint32_t* groups, int64_t first_row, int64_t n_rows) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    h->trk.stale = true;          // (frp.h, face tracks: a cached match must not outlive a change of the rows; set even where the call then fails)
    FRPCHK(refuse_while_reserved(h));
    if (!groups || first_row < 0 || n_rows < 0 || first_row + n_rows > h->g_rows) return fail(h, FRP_ERR_INVALID, "bad gallery range");
    std::copy(groups, groups + n_rows, h->g_groups.begin() + first_row);
    return push_groups(h, first_row, n_rows);
}

int frp_gallery_get_groups(frp_handle* h, uint32_t* out, int64_t first_row, int64_t n_rows) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!out || first_row < 0 || n_rows < 0 || first_row + n_rows > h->g_rows) return fail(h, FRP_ERR_INVALID, "bad gallery range");
    std::copy(h->g_groups.begin() + first_row, h->g_groups.begin() + first_row + n_rows, out);
    return FRP_OK;
}

int frp_gallery_exact(frp_handle* h, int32_t on) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    h->trk.stale = true;          // (frp.h, face tracks: a cached match must not outlive a change of the rows; set even where the call then fails)
    if (!on) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        release(h->gx); release(h->gx_q); release(h->gx_out);
        h->g_exact = false;
        return FRP_OK;
    }
    if (h->g_exact) return FRP_OK;
    // rows that exist already: the unit fp16 rows widened (their exact values are gone), with room for the snapshot's row capacity
    ScopedBuf fresh;
    const size_t cap_rows = std::max<size_t>(h->gallery.cap / ((size_t)FRP_EMB_DIM * 2), (size_t)h->g_rows);
    FRPCHK(exact_from_f16(h, h->gallery.p, h->g_rows, cap_rows, fresh));
    release(h->gx);
    h->gx = fresh.take();
    h->g_exact = true;
    return FRP_OK;
}

int frp_gallery_distances(frp_handle* h, const double* q, int32_t M, double* dist, int64_t n_cols) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!h->g_exact) return fail(h, FRP_ERR_INVALID, "exact rows are not enabled (frp_gallery_exact)");
    if (!q || !dist || M <= 0 || M > 65536) return fail(h, FRP_ERR_INVALID, "bad distance arguments");
    if (n_cols != h->g_rows) return fail(h, FRP_ERR_INVALID, "gallery_distances: output sized for another gallery size");
    if (h->g_rows == 0) return FRP_OK;
    FRPCHK(ensure(h, h->gx_q, (size_t)M * FRP_EMB_DIM * 8));
    FRPCHK(ensure(h, h->gx_out, (size_t)M * h->g_rows * 8));
    HIPCHK(h, hipMemcpyAsync(h->gx_q.p, q, (size_t)M * FRP_EMB_DIM * 8, hipMemcpyHostToDevice, h->stream));
    hipError_t e = launch_gallery_distances((const double*)h->gx.p, h->g_rows, (const double*)h->gx_q.p, M, (double*)h->gx_out.p, h->stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("gallery_distances: ") + hipGetErrorString(e));
    HIPCHK(h, hipMemcpyAsync(dist, h->gx_out.p, (size_t)M * h->g_rows * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return FRP_OK;
}

int frp_gallery_get_exact(frp_handle* h, double* out, int64_t first_row, int64_t n_rows) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!h->g_exact) return fail(h, FRP_ERR_INVALID, "exact rows are not enabled (frp_gallery_exact)");
    if (!out || first_row < 0 || n_rows < 0 || first_row + n_rows > h->g_rows) return fail(h, FRP_ERR_INVALID, "bad gallery range");
    if (n_rows == 0) return FRP_OK;
    HIPCHK(h, hipMemcpyAsync(out, (double*)h->gx.p + first_row * FRP_EMB_DIM, (size_t)n_rows * FRP_EMB_DIM * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return FRP_OK;
}

}  // extern "C"
