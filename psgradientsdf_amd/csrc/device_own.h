// device_own.h -- who frees what: the owners of the device and pinned host memory a context (engine_internal.h psgsdf_ctx) or a call holds.
// Needs the HIP runtime API alone (no kernel header), so that a host-only program can include it (tests/test_host_tools.py).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

namespace psge {

// One array of T, freed when its owner goes.  Converts to T*, so everything that only reads the pointer is written as for a raw one.
// alloc frees what is held, then allocates sizeof(T) * count bytes; on failure the error comes back and the buffer is empty.
struct DevKind { static hipError_t get(void** p, size_t bytes) { return hipMalloc(p, bytes); } static hipError_t put(void* p) { return hipFree(p); } };
struct PinKind { static hipError_t get(void** p, size_t bytes, unsigned flags = hipHostMallocDefault) { return hipHostMalloc(p, bytes, flags); } static hipError_t put(void* p) { return hipHostFree(p); } };
template <class T, class Kind> struct OwnedBuf {
    OwnedBuf() = default;
    OwnedBuf(const OwnedBuf&) = delete;
    OwnedBuf& operator=(const OwnedBuf&) = delete;
    OwnedBuf(OwnedBuf&& o) noexcept : p(o.release()) {}
    OwnedBuf& operator=(OwnedBuf&& o) noexcept { if (this != &o) adopt(o.release()); return *this; }
    ~OwnedBuf() { reset(); }
    operator T*() const { return p; }
    template <class... Flags> hipError_t alloc(size_t count, Flags... flags) {
        reset();
        const hipError_t e = Kind::get((void**)&p, sizeof(T) * count, flags...);
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    void adopt(void* q) { reset(); p = (T*)q; }      // memory somebody else chose the kind of (comm.hip xr_alloc)
    void reset() { if (p) (void)Kind::put(p); p = nullptr; }
    T* release() { T* q = p; p = nullptr; return q; }   // gives the memory up WITHOUT freeing it (psgsdf_destroy: exported memory a peer may still map)
private:
    T* p = nullptr;
};
template <class T> using DevBuf = OwnedBuf<T, DevKind>;      // device array
template <class T> using PinBuf = OwnedBuf<T, PinKind>;      // pinned host array; alloc(count, hipHostMallocMapped) for the mailbox kernels write into

// The planes of a dense grid and the view of them the kernels take (V = engine.h DenseView: dist, g[3], rho[3], weight, vis with KW words
// per voxel, row_of) in ONE object: there is no second copy of the pointers that an allocation or a free could forget.
template <class V> struct DensePlanesOf : V {
    DensePlanesOf() : V{} {}
    DensePlanesOf(const DensePlanesOf&) = delete;
    DensePlanesOf& operator=(const DensePlanesOf&) = delete;
    DensePlanesOf(DensePlanesOf&& o) noexcept : V(o) { static_cast<V&>(o) = V{}; }
    DensePlanesOf& operator=(DensePlanesOf&& o) noexcept { if (this != &o) { reset(); static_cast<V&>(*this) = o; static_cast<V&>(o) = V{}; } return *this; }
    ~DensePlanesOf() { reset(); }
    // every plane of nvox voxels (vis only if KW > 0, row_of only if asked for) -- or, if one allocation fails, none
    hipError_t alloc(long long nvox, int KW, bool with_rowof) {
        reset();
        hipError_t e = one(&this->dist, nvox);
        for (int a = 0; a < 3; ++a) { if (e == hipSuccess) e = one(&this->g[a], nvox); if (e == hipSuccess) e = one(&this->rho[a], nvox); }
        if (e == hipSuccess) e = one(&this->weight, nvox);
        if (e == hipSuccess && KW > 0) e = one(&this->vis, nvox * KW);
        if (e == hipSuccess && with_rowof) e = one(&this->row_of, nvox);
        if (e != hipSuccess) reset(); else this->KW = KW;
        return e;
    }
    // the visibility plane alone, for another number of words per voxel (psgsdf_init: the keyframes are known)
    hipError_t alloc_vis(long long nvox, int KW) {
        if (this->vis) (void)hipFree(this->vis);
        this->vis = nullptr;
        const hipError_t e = one(&this->vis, nvox * KW);
        if (e == hipSuccess) this->KW = KW;
        return e;
    }
    void reset() {
        void* const all[] = {this->dist, this->g[0], this->g[1], this->g[2], this->rho[0], this->rho[1], this->rho[2], this->weight, this->vis, this->row_of};
        for (void* q : all) if (q) (void)hipFree(q);
        static_cast<V&>(*this) = V{};
    }
private:
    template <class T> static hipError_t one(T** p, long long count) {
        const hipError_t e = hipMalloc((void**)p, sizeof(T) * (size_t)count);
        if (e != hipSuccess) *p = nullptr;
        return e;
    }
};

}  // namespace psge
