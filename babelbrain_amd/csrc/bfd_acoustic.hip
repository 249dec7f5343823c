// An acoustic study on MI355X: the volumes of one Step-2 calculation (TranscranialModeling/BabelIntegrationBASE.py:1840-2201, 2321-2520, 2729-2885)
// held on the device from their one upload to the results the caller asks for. The arithmetic is the existing entries': the label survey and the map
// assembly (bfd_domain.hip), the engine's device-pointer setters (bfd_api.hip) and the result packing (bfd_pack.hip) run here through their stages
// (bfd_domain_stages.h), the same launch sequences their public entries run between their own copies, so every result equals what the separate calls
// give, element by element. This file adds no kernel: it owns the memory, orders the stages and counts the bytes that cross the host boundary.
// Stages on resident volumes run on the null stream and end with a read-back of their few result words, so the engine's own stream, which waits for
// no other, finds the map complete; the pack runs on the engine's stream and is waited for before the call returns.
#include <limits.h>
#include <string.h>
#include <vector>
#include "bfd_internal.h"
#include "bfd_call.h"
#include "bfd_domain_stages.h"
#include "../../include/babelfdtd.h"

struct bfd_acoustic_s {
    int device = 0, ctBytes = 0; bool hasAir = false;
    int64_t M[3] = {0, 0, 0};
    size_t n = 0, np = 0;                            // voxels of the label volume; rounded up to whole 32-bit words
    uint8_t *labels = nullptr, *air = nullptr; void *ct = nullptr;
    unsigned long long *hist = nullptr, *c64 = nullptr; int *bnd = nullptr; unsigned *first = nullptr, *c32 = nullptr; uint32_t *lut = nullptr;
    bool volumes = false, assembled = false, haveNoCT = false, haveAir = false;
    int64_t N[3] = {0, 0, 0};
    size_t mapCap = 0;                               // voxels the three map volumes hold
    uint32_t *map = nullptr, *mapNoCT = nullptr, *airOut = nullptr;
    struct Slot {
        bool packed = false, haveNoCT = false, haveAir = false, haveMap = false;
        int O[3] = {0, 0, 0}; size_t cap = 0;
        float *amp = nullptr, *cplx = nullptr, *peak = nullptr; uint32_t *mm = nullptr, *mmNoCT = nullptr; uint8_t *airMask = nullptr;
    } slot[3];
    int64_t up = 0, down = 0;
};

namespace {

hipError_t copy_up(bfd_acoustic_s *s, void *dst, const void *src, size_t bytes)
{
    s->up += (int64_t)bytes;
    return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
}
hipError_t copy_down(bfd_acoustic_s *s, void *dst, const void *src, size_t bytes)
{
    s->down += (int64_t)bytes;
    return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
}
template <typename T> void release(T *&p) { if (p) hipFree(p); p = nullptr; }
template <typename T> hipError_t hold(T *&p, size_t count) { return hipMalloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T)); }

void release_slot(bfd_acoustic_s::Slot &t)
{
    release(t.amp); release(t.cplx); release(t.peak); release(t.mm); release(t.mmNoCT); release(t.airMask);
    t = bfd_acoustic_s::Slot();
}

}  // namespace

extern "C" int bfd_acoustic_create(int device, int64_t M1, int64_t M2, int64_t M3, int ctBytes, int hasAir, bfd_acoustic *handle)
{
    static const char *who = "bfd_acoustic_create";
    if (!handle) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (M1 < 1 || M2 < 1 || M3 < 1) BFD_FAIL(-1, std::string(who) + ": every dimension must be at least 1");
    if (!volume_fits(M1, M2, M3)) BFD_FAIL(-1, std::string(who) + ": the volume has 2^31 voxels or more (limit: fewer than 2^31)");
    if (ctBytes != 0 && ctBytes != 2 && ctBytes != 4) BFD_FAIL(-1, std::string(who) + ": ctBytes must be 0, 2 or 4");
    if (hasAir != 0 && hasAir != 1) BFD_FAIL(-1, std::string(who) + ": hasAir must be 0 or 1");
    if (hasAir && !ctBytes) BFD_FAIL(-1, std::string(who) + ": the air mask is read with a ct only");
    if (int rc = pick_device(who, device)) return rc;
    bfd_acoustic_s *s = new bfd_acoustic_s;
    s->device = device; s->ctBytes = ctBytes; s->hasAir = hasAir != 0;
    s->M[0] = M1; s->M[1] = M2; s->M[2] = M3;
    s->n = (size_t)(M1 * M2 * M3); s->np = (s->n + 3) / 4 * 4;
    hipError_t e = hold(s->labels, s->np);
    if (e == hipSuccess) e = hipMemset(s->labels, 0, s->np);
    if (e == hipSuccess && ctBytes) e = hipMalloc(&s->ct, s->n * (size_t)ctBytes);
    if (e == hipSuccess && hasAir) e = hold(s->air, s->n);
    if (e == hipSuccess) e = hold(s->hist, 257);
    if (e == hipSuccess) e = hold(s->bnd, 6);
    if (e == hipSuccess) e = hold(s->first, 1);
    if (e == hipSuccess) e = hold(s->c64, 3);
    if (e == hipSuccess) e = hold(s->c32, 5);
    if (e == hipSuccess) e = hold(s->lut, 256);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        bfd_acoustic_destroy(s);
        BFD_FAIL(-10, std::string(who) + ": " + hipGetErrorString(e));
    }
    *handle = s;
    return 0;
}

extern "C" void bfd_acoustic_destroy(bfd_acoustic s)
{
    if (!s) return;
    if (hipSetDevice(s->device) == hipSuccess) hipDeviceSynchronize();
    release(s->labels); release(s->air); if (s->ct) hipFree(s->ct);
    release(s->hist); release(s->bnd); release(s->first); release(s->c64); release(s->c32); release(s->lut);
    release(s->map); release(s->mapNoCT); release(s->airOut);
    for (auto &t : s->slot) release_slot(t);
    delete s;
}

extern "C" int bfd_acoustic_set_volumes(bfd_acoustic s, const uint8_t *labels, const void *ct, const uint8_t *air)
{
    static const char *who = "bfd_acoustic_set_volumes";
    if (!s || !labels) BFD_FAIL(-1, std::string(who) + ": null argument");
    if ((s->ctBytes != 0) != (ct != nullptr)) BFD_FAIL(-1, std::string(who) + ": a ct is passed where the study was created for one, and only there");
    if (s->hasAir != (air != nullptr)) BFD_FAIL(-1, std::string(who) + ": an air mask is passed where the study was created for one, and only there");
    if (int rc = pick_device(who, s->device)) return rc;
    s->volumes = s->assembled = false;
    BFD_STEP(copy_up(s, s->labels, labels, s->n));
    if (ct) BFD_STEP(copy_up(s, s->ct, ct, s->n * (size_t)s->ctBytes));
    if (air) BFD_STEP(copy_up(s, s->air, air, s->n));
    s->volumes = true;
    return 0;
}

extern "C" int bfd_acoustic_survey(bfd_acoustic s, const int64_t *lo, const int64_t *hi, int flipK, int64_t *hist, int64_t *bounds, int64_t *focal)
{
    static const char *who = "bfd_acoustic_survey";
    if (!s || !lo || !hi || !hist || !bounds || !focal) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (int rc = bfd_survey_arguments(who, s->M[0], s->M[1], s->M[2], lo, hi, flipK)) return rc;
    if (!s->volumes) BFD_FAIL(-6, std::string(who) + ": bfd_acoustic_set_volumes comes first");
    if (int rc = pick_device(who, s->device)) return rc;
    unsigned long long h[257];
    int bnd[6] = {INT_MAX, -1, INT_MAX, -1, INT_MAX, -1};
    unsigned first = 0xFFFFFFFFu;
    BFD_STEP(hipMemset(s->hist, 0, sizeof h));
    BFD_STEP(copy_up(s, s->bnd, bnd, sizeof bnd));
    BFD_STEP(copy_up(s, s->first, &first, sizeof first));
    BFD_STEP(bfd_stage_label_survey(s->labels, s->M[0], s->M[1], s->M[2], lo, hi, flipK, s->hist, s->bnd, s->first));
    BFD_STEP(copy_down(s, h, s->hist, sizeof h));
    BFD_STEP(copy_down(s, bnd, s->bnd, sizeof bnd));
    BFD_STEP(copy_down(s, &first, s->first, sizeof first));
    bfd_label_survey_finish(h, bnd, first, hist, bounds, focal);
    return 0;
}

extern "C" int bfd_acoustic_assemble(bfd_acoustic s, const int64_t *lo, const int64_t *size, const int64_t *padLo, const int64_t *padHi, int flipK,
                                     const uint32_t *lut, uint32_t ctOffset, int64_t zWater, int64_t nMaterials, const int64_t *focalIJ, int waterOnly,
                                     int64_t *stats)
{
    static const char *who = "bfd_acoustic_assemble";
    if (!s || !lo || !size || !padLo || !padHi || !lut || !focalIJ || !stats) BFD_FAIL(-1, std::string(who) + ": null argument");
    int64_t N[3];
    if (int rc = bfd_assemble_arguments(who, s->M[0], s->M[1], s->M[2], s->ctBytes != 0, lo, size, padLo, padHi, flipK, lut, zWater, nMaterials, focalIJ, N)) return rc;
    if (waterOnly != 0 && waterOnly != 1) BFD_FAIL(-1, std::string(who) + ": waterOnly must be 0 or 1");
    const size_t nOut = (size_t)(N[0] * N[1] * N[2]);
    if (!nOut) BFD_FAIL(-1, std::string(who) + ": the map has no voxel");
    if (!s->volumes) BFD_FAIL(-6, std::string(who) + ": bfd_acoustic_set_volumes comes first");
    if (int rc = pick_device(who, s->device)) return rc;
    s->assembled = false;
    if (nOut > s->mapCap) {
        release(s->map); release(s->mapNoCT); release(s->airOut);
        s->mapCap = 0;
        BFD_STEP(hold(s->map, nOut));
        if (s->ctBytes) BFD_STEP(hold(s->mapNoCT, nOut));
        if (s->hasAir) BFD_STEP(hold(s->airOut, nOut));
        s->mapCap = nOut;
    }
    for (int q = 0; q < 3; q++) s->N[q] = N[q];
    if (waterOnly) {                                  // :2203: the map is all water, nothing else exists
        BFD_STEP(hipMemset(s->map, 0, 4 * nOut));
        BFD_STEP(hipDeviceSynchronize());
        s->haveNoCT = s->haveAir = false;
        stats[0] = 0; stats[1] = stats[2] = -1; stats[3] = stats[4] = 0; stats[5] = stats[6] = -1; stats[7] = 0;
        s->assembled = true;
        return 0;
    }
    unsigned long long c64[3] = {0, 0, 0};
    unsigned c32[5] = {0xFFFFFFFFu, 0u, 0u, 0x7FFFFFFFu, 0x7FFFFFFFu};
    BFD_STEP(copy_up(s, s->lut, lut, 256 * sizeof(uint32_t)));
    BFD_STEP(copy_up(s, s->c64, c64, sizeof c64));
    BFD_STEP(copy_up(s, s->c32, c32, sizeof c32));
    BFD_STEP(bfd_stage_assemble_map(s->labels, s->ct, s->ctBytes, s->air, s->M[1], s->M[2], N, lo, size, padLo, flipK, s->lut, ctOffset, zWater, nMaterials,
                                    focalIJ, s->map, s->mapNoCT, s->airOut, s->c64, s->c32));
    BFD_STEP(copy_down(s, c64, s->c64, sizeof c64));
    BFD_STEP(copy_down(s, c32, s->c32, sizeof c32));
    bfd_assemble_finish(c64, c32, stats);
    s->haveNoCT = s->ctBytes != 0; s->haveAir = s->hasAir;
    s->assembled = true;
    return 0;
}

// the sim is a whole domain of the map's shape on the study's device
static int sim_fits(const bfd_acoustic_s *s, const bfd_sim *sim, const char *who)
{
    if (sim->cfg.device != s->device) BFD_FAIL(-1, std::string(who) + ": the sim is on another device than the study");
    if (sim->d.k0 != 0 || sim->d.N1 != s->N[0] || sim->d.N2 != s->N[1] || sim->d.nk != s->N[2] || sim->d.N3 != s->N[2])
        BFD_FAIL(-1, std::string(who) + ": the sim is not a whole domain of the assembled map's shape");
    return 0;
}

extern "C" int bfd_acoustic_attach(bfd_acoustic s, bfd_sim *sim)
{
    static const char *who = "bfd_acoustic_attach";
    if (!s || !sim) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (!s->assembled) BFD_FAIL(-6, std::string(who) + ": bfd_acoustic_assemble comes first");
    if (int rc = sim_fits(s, sim, who)) return rc;
    const int64_t s1 = s->N[1] * s->N[2], s2 = s->N[2];
    if (int rc = bfd_set_material_map_device(sim, s->map, s1, s2, 1, 0, 0)) return rc;
    if (s->haveAir) return bfd_set_reflector_device(sim, s->airOut, s1, s2, 1);
    return 0;
}

extern "C" int bfd_acoustic_pack(bfd_acoustic s, bfd_sim *sim, const bfd_pack_spec *spec, int slot)
{
    static const char *who = "bfd_acoustic_pack";
    if (!s) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (slot < 0 || slot > 2) BFD_FAIL(-1, std::string(who) + ": slot must be 0 (tissue), 1 (water) or 2 (refocus)");
    if (int rc = bfd_pack_arguments(who, sim, spec, true, true)) return rc;
    if (!s->assembled) BFD_FAIL(-6, std::string(who) + ": bfd_acoustic_assemble comes first");
    if (int rc = sim_fits(s, sim, who)) return rc;
    if (bfd_current_step(sim) <= 0) BFD_FAIL(-6, std::string(who) + ": the run comes first (the sim is at step 0)");
    if (int rc = pick_device(who, s->device)) return rc;
    bfd_acoustic_s::Slot &t = s->slot[slot];
    const size_t nOut = (size_t)spec->O[0] * spec->O[1] * spec->O[2];
    t.packed = false;
    if (nOut > t.cap) {
        release_slot(t);
        BFD_STEP(hold(t.amp, nOut)); BFD_STEP(hold(t.cplx, 2 * nOut)); BFD_STEP(hold(t.peak, nOut));
        BFD_STEP(hold(t.mm, nOut));
        if (s->ctBytes) BFD_STEP(hold(t.mmNoCT, nOut));
        if (s->hasAir) BFD_STEP(hold(t.airMask, nOut));
        t.cap = nOut;
    }
    for (int q = 0; q < 3; q++) t.O[q] = spec->O[q];
    if (int rc = bfd_stage_pack_results(sim, spec, t.amp, t.cplx, t.peak)) return rc;
    BFD_STEP(bfd_stage_pack_map(sim, spec, s->map, t.mm, 4));
    if (s->haveNoCT) BFD_STEP(bfd_stage_pack_map(sim, spec, s->mapNoCT, t.mmNoCT, 4));
    if (s->haveAir) BFD_STEP(bfd_stage_pack_map(sim, spec, s->airOut, t.airMask, 1));
    if (int rc = bfd_sync(sim)) return rc;
    t.haveMap = true; t.haveNoCT = s->haveNoCT; t.haveAir = s->haveAir;
    t.packed = true;
    return 0;
}

extern "C" int bfd_acoustic_get(bfd_acoustic s, int which, int slot, void *out)
{
    static const char *who = "bfd_acoustic_get";
    if (!s || !out) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (which < BFD_ACOUSTIC_P_AMP || which > BFD_ACOUSTIC_FULL_AIR) BFD_FAIL(-1, std::string(who) + ": which is not a result of the study");
    const bool full = which >= BFD_ACOUSTIC_FULL_MAP;
    if (!full && (slot < 0 || slot > 2)) BFD_FAIL(-1, std::string(who) + ": slot must be 0 (tissue), 1 (water) or 2 (refocus)");
    const void *src = nullptr; size_t bytes = 0;
    if (full) {
        if (!s->assembled) BFD_FAIL(-6, std::string(who) + ": bfd_acoustic_assemble comes first");
        const size_t nMap = (size_t)(s->N[0] * s->N[1] * s->N[2]);
        if (which == BFD_ACOUSTIC_FULL_MAP) src = s->map;
        else if (which == BFD_ACOUSTIC_FULL_MAP_NOCT) src = s->haveNoCT ? s->mapNoCT : nullptr;
        else src = s->haveAir ? s->airOut : nullptr;
        bytes = 4 * nMap;
    } else {
        const bfd_acoustic_s::Slot &t = s->slot[slot];
        if (!t.packed) BFD_FAIL(-6, std::string(who) + ": bfd_acoustic_pack of this slot comes first");
        const size_t nOut = (size_t)t.O[0] * t.O[1] * t.O[2];
        switch (which) {
        case BFD_ACOUSTIC_P_AMP: src = t.amp; bytes = 4 * nOut; break;
        case BFD_ACOUSTIC_P_COMPLEX: src = t.cplx; bytes = 8 * nOut; break;
        case BFD_ACOUSTIC_PEAK: src = t.peak; bytes = 4 * nOut; break;
        case BFD_ACOUSTIC_MATERIAL_MAP: src = t.mm; bytes = 4 * nOut; break;
        case BFD_ACOUSTIC_MATERIAL_MAP_NOCT: src = t.haveNoCT ? t.mmNoCT : nullptr; bytes = 4 * nOut; break;
        default: src = t.haveAir ? t.airMask : nullptr; bytes = nOut; break;
        }
    }
    if (!src) BFD_FAIL(-6, std::string(who) + ": the study holds no such volume (no ct, no air mask, or a water-only map)");
    if (int rc = pick_device(who, s->device)) return rc;
    BFD_STEP(copy_down(s, out, src, bytes));
    return 0;
}

extern "C" int bfd_acoustic_traffic(bfd_acoustic s, int64_t *bytesUp, int64_t *bytesDown)
{
    if (!s || !bytesUp || !bytesDown) BFD_FAIL(-1, "bfd_acoustic_traffic: null argument");
    *bytesUp = s->up; *bytesDown = s->down;
    return 0;
}
