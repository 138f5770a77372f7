// mc_context_bind_mandelbrot_orbit_tables: the BLA tables of precisions 4 and 5 built on the device, straight into the binding's
// buffers, from the orbit table the bind has just uploaded (include/mc_compute.h).
//
//  * the arithmetic is mandel_bla_table.h's, the text the host builders run: a level-0 entry from Z_j, an entry of level k from the two
//    adjacent entries of level k - 1.  Entries of one level are independent; levels depend on each other.
//  * one kernel.  A workgroup owns kBlaGroupEntries = 2^c consecutive entries of the launch's first level and everything above them that
//    depends on nothing else: 2^(c-1) entries of the next level, ... one entry c levels up, with a block barrier between levels (the
//    entries are read back from the table in device memory, between a release and an acquire fence).  So a launch builds c + 1
//    levels, and from the first level of at most kBlaGroupEntries entries down to the table's last everything runs in a single
//    workgroup: 18 levels (L = 200 000) are two launches, any table at most three.
//  * memory bound and short: one lane per entry, 16 B read per level-0 entry, two records read and one written per entry above; no LDS,
//    no atomics.  256 threads per workgroup (four waves, one per SIMD) hold four level-0 entries each.
//  * IEEE double in source order (-ffp-contract=off), fp64 denormals kept.
#include "mandel_bla_table.h"
#include "mandel_perturb.h"
#include "mandel_side_record.h"
#include "mc_internal.h"

namespace mc {

namespace {

constexpr uint32_t kBlaGroupEntries = MC_BLA_TABLE_GROUP_ENTRIES;
constexpr uint32_t kBlaThreads = 256;
constexpr uint32_t kBlaGroupLevels = 11;   // log2(kBlaGroupEntries) + 1: the levels one launch builds
static_assert(kBlaGroupEntries == 1u << (kBlaGroupLevels - 1), "a group halves down to one entry");

// MC_PRECISION_PERTURB_BLA: five doubles per entry.
struct PlainTable {
    using Rec = double;   // the table's element; an entry is kPlainDoubles of them
    using Cm = double;
    static constexpr size_t kEntryBytes = blatab::kPlainDoubles * sizeof(double);
    static __device__ __forceinline__ void level0(double2 z, Rec* t, uint64_t at) {
        double e[blatab::kPlainDoubles];
        blatab::plain_level0(z.x, z.y, e);
        for (int i = 0; i < blatab::kPlainDoubles; i++) t[blatab::kPlainDoubles * at + i] = e[i];
    }
    static __device__ __forceinline__ void merge(Rec* t, uint64_t x_at, uint64_t at, const Cm& cm) {
        double x[blatab::kPlainDoubles], y[blatab::kPlainDoubles], e[blatab::kPlainDoubles];
        for (int i = 0; i < blatab::kPlainDoubles; i++) {
            x[i] = t[blatab::kPlainDoubles * x_at + i];
            y[i] = t[blatab::kPlainDoubles * (x_at + 1) + i];
        }
        blatab::plain_merge(x, y, cm, e);
        for (int i = 0; i < blatab::kPlainDoubles; i++) t[blatab::kPlainDoubles * at + i] = e[i];
    }
};

// MC_PRECISION_PERTURB_BLA_DEEP: one 64-byte record per entry.
struct DeepTable {
    using Rec = BlaDeepRec;
    using Cm = blatab::Fx;
    static constexpr size_t kEntryBytes = sizeof(BlaDeepRec);
    static __device__ __forceinline__ void level0(double2 z, Rec* t, uint64_t at) {
        BlaDeepRec r;
        blatab::deep_level0(z.x, z.y, r);
        t[at] = r;
    }
    static __device__ __forceinline__ void merge(Rec* t, uint64_t x_at, uint64_t at, const Cm& cm) {
        const BlaDeepRec x = t[x_at], y = t[x_at + 1];
        BlaDeepRec r;
        blatab::deep_merge(x, y, cm, r);
        t[at] = r;
    }
};

// Levels first .. first + kBlaGroupLevels - 1 (as far as the table has them).  off: where level `first` starts in the table, below: where
// level first - 1 does (unused at first = 0, whose entries come from Z).  Every index is below the table's entry count: q < n0 >> k.
template <class T>
__global__ void __launch_bounds__(kBlaThreads) mandel_bla_table_kernel(const double2* __restrict__ Z, typename T::Rec* table, uint64_t n0,
                                                                       uint32_t first, uint32_t levels, uint64_t off, uint64_t below,
                                                                       typename T::Cm cm) {
    uint64_t cnt = n0 >> first;
    uint64_t base = (uint64_t)blockIdx.x * kBlaGroupEntries;   // the group's first entry of the level, and how many it owns
    uint32_t width = kBlaGroupEntries;
    for (uint32_t k = first; k < levels && width >= 1u; k++) {   // uniform over the workgroup
        const uint64_t end = base + width < cnt ? base + width : cnt;
        for (uint64_t q = base + threadIdx.x; q < end; q += kBlaThreads) {
            if (k == 0u) T::level0(Z[q + 1u], table, q);           // step j = q + 1 <= L - 2
            else T::merge(table, below + 2u * q, off + q, cm);     // (k-1, 2q) and (k-1, 2q + 1): this group's own, or an earlier launch's
        }
        // The next level reads what this one stored, through device memory.  __syncthreads() alone orders LDS only, so the stores are
        // released and the loads acquired explicitly (agent scope: the stores have left the wave and no stale line is read back).
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        below = off;
        off += cnt;
        cnt >>= 1;
        base >>= 1;
        width >>= 1;
    }
}

template <class T>
int build_table(const double2* d_orbit, void* d_table, const blatab::Shape& sh, const typename T::Cm& cm, hipStream_t s, uint32_t* launches) {
    uint64_t off = 0, below = 0;
    for (uint32_t first = 0; first < sh.levels; first += kBlaGroupLevels) {
        const uint64_t cnt = sh.n0 >> first;
        const uint64_t groups = (cnt + kBlaGroupEntries - 1u) / kBlaGroupEntries;
        hipLaunchKernelGGL(mandel_bla_table_kernel<T>, dim3((uint32_t)groups), dim3(kBlaThreads), 0, s, d_orbit,
                           (typename T::Rec*)d_table, sh.n0, first, sh.levels, off, below, cm);
        MC_HIP_TRY(hipGetLastError());
        (*launches)++;
        for (uint32_t k = first; k < first + kBlaGroupLevels && k < sh.levels; k++) {
            below = off;
            off += sh.n0 >> k;
        }
    }
    return MC_OK;
}

struct TableDevice {
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool valid = false;
    double device_ms = 0.0;
    uint32_t launches = 0;
};
SideRecords<TableDevice> g_table_devices;

}  // namespace

size_t bla_table_bytes(uint32_t table, uint32_t length) {
    const blatab::Shape sh = blatab::shape(length);
    return (size_t)sh.total * (table == MC_ORBIT_TABLE_BLA ? PlainTable::kEntryBytes : DeepTable::kEntryBytes);
}

int bla_table_build(mc_context* ctx, uint32_t tables, const void* d_orbit, uint32_t length, double scale_x, double scale_y, bool deep,
                    int32_t scale_exp2, void* d_bla, void* d_bla_deep, hipStream_t s) {
    TableDevice* d = g_table_devices.get(ctx);
    d->valid = false;
    for (auto& e : d->ev)
        if (!e) MC_HIP_TRY(hipEventCreate(&e));
    const blatab::Shape sh = blatab::shape(length);
    uint32_t launches = 0;
    int rc = MC_OK;
    MC_HIP_TRY(hipEventRecord(d->ev[0], s));
    if (sh.total && (tables & MC_ORBIT_TABLE_BLA) &&
        (rc = build_table<PlainTable>((const double2*)d_orbit, d_bla, sh, blatab::plain_cm(scale_x, scale_y), s, &launches)))
        return rc;
    if (sh.total && (tables & MC_ORBIT_TABLE_BLA_DEEP) &&
        (rc = build_table<DeepTable>((const double2*)d_orbit, d_bla_deep, sh, blatab::deep_cm(scale_x, scale_y, deep, scale_exp2), s,
                                     &launches)))
        return rc;
    MC_HIP_TRY(hipEventRecord(d->ev[1], s));
    MC_HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.0f;
    MC_HIP_TRY(hipEventElapsedTime(&ms, d->ev[0], d->ev[1]));
    d->device_ms = launches ? ms : 0.0;
    d->launches = launches;
    d->valid = true;
    return MC_OK;
}

void bla_table_release(mc_context* ctx) {
    g_table_devices.erase(ctx, [](TableDevice& d) {
        for (auto& e : d.ev)
            if (e) (void)hipEventDestroy(e);
    });
}

}  // namespace mc

extern "C" int mc_context_last_table_timing(mc_context* ctx, double* device_ms, uint32_t* launches) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    const mc::TableDevice* d = mc::g_table_devices.find(ctx);
    if (!d || !d->valid) return MC_ERR_INVALID_ARGUMENT;
    if (device_ms) *device_ms = d->device_ms;
    if (launches) *launches = d->launches;
    return MC_OK;
}
