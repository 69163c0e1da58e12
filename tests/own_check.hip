// The owners of device and pinned memory (csrc/device_own.h) on the paths a green run never takes: every allocation here is one no device can
// serve (2^62 bytes; without a device the runtime refuses anything), and the moves are done on an address that is never dereferenced or freed.
// Built with the host sanitizers and run by tests/test_host_tools.py.
#include "device_own.h"
#include "engine.h"
#include <stdio.h>
#include <utility>
#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)
using namespace psge;
typedef DensePlanesOf<psg::DenseView> DensePlanes;

int main() {
    { DevBuf<double> d; PinBuf<double> p; }                    // destruction of empty buffers
    {   // move, release: on an address that must never reach hipFree
        double* const fake = (double*)(size_t)4096;
        DevBuf<double> a; a.adopt(fake);
        DevBuf<double> b(std::move(a)); CHECK(!a && b == fake);
        PinBuf<double> p; p.adopt(fake);
        PinBuf<double> q; q = std::move(p); CHECK(!p && q == fake && q + 2 == fake + 2);
        CHECK(b.release() == fake && !b && q.release() == fake && !q && b.release() == nullptr);
    }
    const size_t huge = (size_t)1 << 59;                       // doubles: 2^62 bytes
    DevBuf<double> d; PinBuf<double> p;
    CHECK(d.alloc(huge) != hipSuccess && !d && p.alloc(huge) != hipSuccess && !p && p.alloc(huge, hipHostMallocMapped) != hipSuccess && !p);
    d.reset(); d.reset(); p.reset();
    DensePlanes planes;
    CHECK(planes.alloc((long long)1 << 60, 2, true) != hipSuccess);      // the first plane already fails: nothing is held
    CHECK(!planes.dist && !planes.g[0] && !planes.g[2] && !planes.rho[1] && !planes.weight && !planes.vis && !planes.row_of && planes.KW == 0);
    planes.reset();
    planes.dist = (float*)(size_t)4096; planes.KW = 3;
    DensePlanes moved(std::move(planes));
    CHECK(!planes.dist && planes.KW == 0 && moved.dist == (float*)(size_t)4096 && moved.KW == 3);
    DensePlanes again; again = std::move(moved);
    CHECK(!moved.dist && again.dist == (float*)(size_t)4096);
    const psg::DenseView& view = again; CHECK(view.dist == again.dist);   // the view IS the owner
    again.dist = nullptr;
    printf("ok\n");
    return 0;
}
