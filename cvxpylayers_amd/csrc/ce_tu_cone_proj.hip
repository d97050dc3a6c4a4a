// translation unit: the stand-alone cone projection and its derivative (k_cone_rows, k_cone_psd, k_cone_dpsd, k_cone_triples, k_cone_dtriples) and the entry
// points that own its handle (ce_cones_create ... ce_cone_dproject).  A projection needs no template matrix, so nothing here touches a ce_handle.
//   (one object file: csrc/Makefile)
#include "ce_tu_prologue.h"
#include <memory>
namespace {
#include "ce_cone_proj.h"
}  // namespace

void ce_set_last_error(const std::string &msg);      // cone_engine.hip: what ce_last_error returns
namespace {
struct ErrSink { void operator=(const std::string &m) const { ce_set_last_error(m); } void operator=(const char *m) const { ce_set_last_error(m); } };
constexpr ErrSink g_err{};
}  // namespace

#define CONE_HIPCHK(call)                                                            \
    do {                                                                             \
        hipError_t e_ = (call);                                                      \
        if (e_ != hipSuccess) {                                                      \
            g_err = std::string(#call) + ": " + hipGetErrorString(e_);               \
            return CE_E_HIP;                                                         \
        }                                                                            \
    } while (0)

struct ce_cones {
    int device = 0;
    ConeProjLayout L{};
    ConeProjDev D{};
    void *dev_mem = nullptr;      // one allocation: the long long, double, int arrays of D in this order
    size_t psd_lds = 0;           // dynamic LDS of the PSD kernels (the footprint of the largest order)
};

int ce_cones_create(int z, int l, int nq, const int *q, int ns, const int *s, int nep, int np, const double *p, int device, ce_cones_handle *out) {
    if (!out || z < 0 || l < 0 || nq < 0 || ns < 0 || nep < 0 || np < 0 || (nq > 0 && !q) || (ns > 0 && !s) || (np > 0 && !p)) { g_err = "ce_cones_create: bad cone description"; return CE_E_BADARG; }
    long long rows = (long long)z + l + 3LL * nep + 3LL * np;
    for (int i = 0; i < nq; i++) { if (q[i] < 1) { g_err = "ce_cones_create: bad SOC dim"; return CE_E_BADARG; } rows += q[i]; }
    for (int i = 0; i < ns; i++) { if (s[i] < 1) { g_err = "ce_cones_create: bad PSD order"; return CE_E_BADARG; } rows += (long long)s[i] * (s[i] + 1) / 2; }
    for (int i = 0; i < np; i++) if (!(fabs(p[i]) > 0.0 && fabs(p[i]) < 1.0)) { g_err = "ce_cones_create: power cone exponent must lie in (-1, 0) or (0, 1)"; return CE_E_BADARG; }
    if (rows <= 0) { g_err = "ce_cones_create: empty cone set"; return CE_E_BADARG; }
    if (rows > 0x7FFFFFFFLL || ns > 65535) { g_err = "ce_cones_create: more than 2^31 - 1 rows or 65535 PSD blocks"; return CE_E_TOO_LARGE; }
    std::vector<int> qoff(nq + 1), soff(ns + 1), small(nq + 1), large(nq + 1);
    std::vector<long long> sstate(ns + 1);
    std::unique_ptr<ce_cones> h(new ce_cones);
    // the LDS footprint is checked before any HIP call
    const int rc = cone_proj_layout(z, l, nq, q, ns, s, nep, np, &h->L, qoff.data(), soff.data(), sstate.data(), small.data(), large.data());
    if (rc > 0) {
        const int k = s[rc - 1];
        g_err = "ce_cones_create: PSD order " + std::to_string(k) + " needs " + std::to_string((long long)cone_proj_psd_lds_doubles(k) * 8) + " bytes of LDS; the largest supported order is " +
                std::to_string(CONE_PROJ_PSD_MAX) + " (" + std::to_string(CONE_PROJ_LDS_BYTES) + " bytes)";
        return CE_E_TOO_LARGE;
    }
    const ConeProjLayout &L = h->L;
    h->device = device;
    h->psd_lds = L.maxs > 0 ? (size_t)cone_proj_psd_lds_doubles(L.maxs) * 8 : 0;
    CONE_HIPCHK(hipSetDevice(device));
    // upload: [sstate (ns) | pw (np) | qoff (nq + 1) | small | large | sord (ns) | soff (ns + 1)]
    const size_t b_ll = sizeof(long long) * (size_t)ns, b_d = sizeof(double) * (size_t)np;
    const size_t n_int = (size_t)(nq + 1) + L.nq_small + L.nq_large + ns + (ns + 1);
    std::vector<char> host(b_ll + b_d + sizeof(int) * n_int);
    if (ns) memcpy(host.data(), sstate.data(), b_ll);
    if (np) memcpy(host.data() + b_ll, p, b_d);
    int *hi = reinterpret_cast<int *>(host.data() + b_ll + b_d);
    size_t o_qoff = 0, o_small = o_qoff + nq + 1, o_large = o_small + L.nq_small, o_sord = o_large + L.nq_large, o_soff = o_sord + ns;
    for (int i = 0; i <= nq; i++) hi[o_qoff + i] = qoff[i];
    for (int i = 0; i < L.nq_small; i++) hi[o_small + i] = small[i];
    for (int i = 0; i < L.nq_large; i++) hi[o_large + i] = large[i];
    for (int i = 0; i < ns; i++) hi[o_sord + i] = s[i];
    for (int i = 0; i <= ns; i++) hi[o_soff + i] = soff[i];
    CONE_HIPCHK(hipMalloc(&h->dev_mem, host.size()));
    hipError_t e = hipMemcpy(h->dev_mem, host.data(), host.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && h->psd_lds > 0) {
        e = ce_set_max_lds(&k_cone_psd, (int)h->psd_lds);
        if (e == hipSuccess) e = ce_set_max_lds(&k_cone_dpsd, (int)h->psd_lds);
    }
    if (e != hipSuccess) { g_err = std::string("ce_cones_create: ") + hipGetErrorString(e); hipFree(h->dev_mem); return CE_E_HIP; }
    char *dm = static_cast<char *>(h->dev_mem);
    const int *di = reinterpret_cast<const int *>(dm + b_ll + b_d);
    ConeProjDev &D = h->D;
    D.z = z; D.l = l; D.nq = nq; D.ns = ns; D.nep = nep; D.np = np;
    D.nq_small = L.nq_small; D.nq_large = L.nq_large; D.e_row0 = L.e_row0;
    D.state_len = L.state_len; D.tri_state0 = L.tri_state0;
    D.sstate = reinterpret_cast<const long long *>(dm); D.pw = reinterpret_cast<const double *>(dm + b_ll);
    D.qoff = di + o_qoff; D.soc_small = di + o_small; D.soc_large = di + o_large; D.sord = di + o_sord; D.soff = di + o_soff;
    *out = h.release();
    return CE_OK;
}

int ce_cones_destroy(ce_cones_handle h) {
    if (!h) return CE_OK;
    hipSetDevice(h->device);
    if (h->dev_mem) hipFree(h->dev_mem);
    delete h;
    return CE_OK;
}

int ce_cones_rows(ce_cones_handle h) { return h ? h->L.m : 0; }
long ce_cones_state_len(ce_cones_handle h) { return h ? (long)h->L.state_len : 0; }

static long long cone_blocks(long long items, int per_block) { return (items + per_block - 1) / per_block; }

// one launch per kind present
static int cone_launch(ce_cones_handle h, bool dproj, ConeProjArgs &a, hipStream_t st) {
    const ConeProjLayout &L = h->L;
    const dim3 nt(CONE_PROJ_NT);
    const long long B = a.B;
    if (B * L.m > (1LL << 40) || B > 0x7FFFFFFFLL / 2) { g_err = "cone projection: batch too large"; return CE_E_TOO_LARGE; }
    CONE_HIPCHK(hipSetDevice(h->device));
    if (L.launch_rows) {
        const long long nbp = cone_blocks(B * (L.z + L.l), CONE_PROJ_NT), nbs = cone_blocks(B * L.nq_small, CONE_PROJ_NT / 16), nbl = cone_blocks(B * L.nq_large, CONE_PROJ_NT / 64);
        if (nbp + nbs + nbl > 0x7FFFFFFFLL) { g_err = "cone projection: batch too large for one grid"; return CE_E_TOO_LARGE; }
        const dim3 grid((unsigned)(nbp + nbs + nbl));
        if (dproj) hipLaunchKernelGGL(k_cone_rows<true>, grid, nt, 0, st, a, (int)nbp, (int)nbs);
        else hipLaunchKernelGGL(k_cone_rows<false>, grid, nt, 0, st, a, (int)nbp, (int)nbs);
    }
    if (L.launch_psd) {
        const dim3 grid((unsigned)B, (unsigned)L.ns);
        if (dproj) hipLaunchKernelGGL(k_cone_dpsd, grid, nt, h->psd_lds, st, a);
        else hipLaunchKernelGGL(k_cone_psd, grid, nt, h->psd_lds, st, a);
    }
    if (L.launch_triples) {
        const long long nb = cone_blocks(B * (L.nep + L.np), CONE_PROJ_NT);
        if (nb > 0x7FFFFFFFLL) { g_err = "cone projection: batch too large for one grid"; return CE_E_TOO_LARGE; }
        if (dproj) hipLaunchKernelGGL(k_cone_dtriples, dim3((unsigned)nb), nt, 0, st, a);
        else hipLaunchKernelGGL(k_cone_triples, dim3((unsigned)nb), nt, 0, st, a);
    }
    CONE_HIPCHK(hipGetLastError());
    return CE_OK;
}

int ce_cone_project(ce_cones_handle h, int B, const double *v, long ld_v, int dual, double *out, long ld_out, double *state, void *stream) {
    if (!h || B <= 0 || !v || !out) { g_err = "null argument"; return CE_E_BADARG; }
    if (ld_v < h->L.m || ld_out < h->L.m) { g_err = "ce_cone_project: a row pitch is smaller than the cone rows"; return CE_E_BADARG; }
    if (out == v) { g_err = "ce_cone_project: out must not alias v"; return CE_E_BADARG; }
    ConeProjArgs a{h->D, B, dual ? 1 : 0, v, ld_v, nullptr, 0, out, ld_out, h->L.state_len > 0 ? state : nullptr};
    return cone_launch(h, false, a, (hipStream_t)stream);
}

int ce_cone_dproject(ce_cones_handle h, int B, const double *v, long ld_v, int dual, const double *state, const double *dir, long ld_dir, double *out, long ld_out, void *stream) {
    if (!h || B <= 0 || !v || !dir || !out || (h->L.state_len > 0 && !state)) { g_err = "null argument"; return CE_E_BADARG; }
    if (ld_v < h->L.m || ld_dir < h->L.m || ld_out < h->L.m) { g_err = "ce_cone_dproject: a row pitch is smaller than the cone rows"; return CE_E_BADARG; }
    if (out == v || out == dir) { g_err = "ce_cone_dproject: out must not alias v or dir"; return CE_E_BADARG; }
    ConeProjArgs a{h->D, B, dual ? 1 : 0, v, ld_v, dir, ld_dir, out, ld_out, const_cast<double *>(state)};
    return cone_launch(h, true, a, (hipStream_t)stream);
}
