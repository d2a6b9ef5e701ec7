// Stand-alone recorder of the conv launch path (tests/test_conv_routes_host.py builds and runs it; no GPU, no Python).
//
// The conv launcher sources are compiled host-only with tests/native/conv_route_shim.h as a forced include, so that a kernel launch
// calls frp_route_record_launch() below instead of the runtime; the handful of HIP runtime entry points the launchers use are
// stubbed here (one device with the CU count given on the command line).  For every case of the case file launch_conv() runs on the
// CPU, and the program prints one JSON line: the return code, the kernel instantiation (the demangled name of its host stub), grid,
// block and LDS bytes, every hipFuncSetAttribute call, and the derived fields of the ConvParams the kernel would have received.
// It needs only launch_conv, ConvParams and the shim: the same source builds against any revision of the launchers.
//
//   conv_route_harness <case file> <CU count>
//   case file: one case per line, "<name> key=value ... ptrs=x,w,bias,out"; keys are the int / float fields of ConvParams
//   (n_cu=-1: the stubbed CU count, as the engine would set it), ptrs lists the pointers that are not null
#include <cxxabi.h>
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "frp_internal.h"

namespace {

int g_ncu = 256;
struct Launch {
    std::string kernel;
    unsigned grid = 0, block = 0;
    size_t lds = 0;
    frp::ConvParams p{};
};
std::vector<Launch> g_launches;
std::vector<std::pair<std::string, int>> g_attrs;

// the symbol at a kernel's host address, "frp::conv_mfma_kernel<256, 128, ...>(frp::ConvParams)" -> "conv_mfma_kernel<256, 128, ...>"
std::string kernel_name(const void* stub) {
    Dl_info info{};
    if (!dladdr(stub, &info) || !info.dli_sname) return "?";
    int status = 0;
    char* dem = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &status);
    std::string s = status == 0 && dem ? dem : info.dli_sname;
    free(dem);
    if (s.rfind("void ", 0) == 0) s = s.substr(5);
    for (const char* pre : {"frp::", "__device_stub__"})
        if (s.rfind(pre, 0) == 0) s = s.substr(strlen(pre));
    const size_t args = s.rfind('(');
    if (args != std::string::npos) s = s.substr(0, args);
    return s;
}

unsigned char g_arena[64 * 16];   // distinct non-null addresses, never dereferenced
template <class T> T* fake(int slot) { return reinterpret_cast<T*>(g_arena + 16 * slot); }

bool set_int(frp::ConvParams& p, const std::string& k, long v) {
#define F(name) if (k == #name) { p.name = (decltype(p.name))v; return true; }
    F(N) F(H) F(W) F(Cin) F(Cout) F(KS) F(stride) F(act) F(flags) F(Hr) F(Wr) F(ksplit) F(Cin2) F(n_cu) F(dbg) F(wino_wide_only)
    F(pf_bytes) F(small_m) F(stem_even_only)
#undef F
    return false;
}

bool set_ptr(frp::ConvParams& p, const std::string& k) {
    int slot = 0;
#define P(name, T) ++slot; if (k == #name) { p.name = fake<T>(slot); return true; }
    P(x, const _Float16) P(w, const _Float16) P(bias, const float) P(slope, const float) P(res, const _Float16) P(x2, const _Float16)
    P(wscale, const float) P(wino_w, const _Float16) P(n_dev, const int32_t) P(stamps, unsigned long long)
    P(stem_x, const _Float16) P(stem_w, const _Float16) P(stem_bias, const float) P(stem_slope, const float) P(stem_out, _Float16)
#undef P
    if (k == "out") { p.out = fake<void>(20); return true; }
    if (k == "out2") { p.out2 = fake<void>(21); return true; }
    if (k == "pf_ptr") { p.pf_ptr = fake<void>(22); return true; }
    return false;
}

void print_record(const std::string& name, const frp::ConvParams& in, int rc) {
    std::ostringstream o;
    o << "{\"case\": \"" << name << "\", \"rc\": " << rc << ", \"launches\": " << g_launches.size() << ", \"attrs\": [";
    for (size_t i = 0; i < g_attrs.size(); ++i) o << (i ? ", " : "") << "[\"" << g_attrs[i].first << "\", " << g_attrs[i].second << "]";
    o << "]";
    if (!g_launches.empty()) {
        const Launch& l = g_launches.back();
        const frp::ConvParams& p = l.p;
        o << ", \"kernel\": \"" << l.kernel << "\", \"grid\": " << l.grid << ", \"block\": " << l.block << ", \"lds\": " << l.lds;
#define D(name) o << ", \"" #name "\": " << (long long)p.name;
        D(pad) D(Ho) D(Wo) D(M) D(Ktot) D(nk) D(cin_shift) D(n_ptiles) D(n_ctiles) D(x_bytes) D(w_bytes) D(x2_bytes) D(x2_shift)
        D(ksplit) D(n_workers) D(n_cu) D(small_m) D(dbg)
#undef D
        o << ", \"stamps_null\": " << (p.stamps ? "false" : "true");
        o << ", \"w_is_wino\": " << (in.wino_w && p.w == in.wino_w ? "true" : "false");
    }
    o << "}";
    std::cout << o.str() << "\n";
}

}  // namespace

extern "C" void frp_route_record_launch(const void* stub, unsigned grid, unsigned block, size_t lds, const void* params, size_t bytes) {
    Launch l;
    l.kernel = kernel_name(stub);
    l.grid = grid; l.block = block; l.lds = lds;
    if (bytes == sizeof(frp::ConvParams)) memcpy(&l.p, params, bytes);
    g_launches.push_back(l);
}

// ---- the HIP runtime entry points the launchers (and the host stubs' registration) reach
extern "C" {
hipError_t hipGetDevice(int* dev) { *dev = 0; return hipSuccess; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t* prop, int) {
    memset(prop, 0, sizeof(*prop));
    prop->multiProcessorCount = g_ncu;
    return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void* func, hipFuncAttribute, int value) {
    g_attrs.emplace_back(kernel_name(func), value);
    return hipSuccess;
}
hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipLaunchKernel(const void*, dim3, dim3, void**, size_t, hipStream_t) { return hipErrorLaunchFailure; }   // (never reached)
void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
void __hipUnregisterFatBinary(void**) {}
hipError_t __hipPopCallConfiguration(dim3*, dim3*, size_t*, hipStream_t*) { return hipSuccess; }
hipError_t __hipPushCallConfiguration(dim3, dim3, size_t, hipStream_t) { return hipSuccess; }
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <case file> <CU count>\n", argv[0]); return 2; }
    g_ncu = atoi(argv[2]);
    std::ifstream f(argv[1]);
    if (!f || g_ncu <= 0) { fprintf(stderr, "bad arguments\n"); return 2; }
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream ls(line);
        std::string name, tok;
        ls >> name;
        frp::ConvParams p{};
        p.in_scale = p.out_scale = 1.0f;
        while (ls >> tok) {
            const size_t eq = tok.find('=');
            const std::string k = tok.substr(0, eq), v = eq == std::string::npos ? "" : tok.substr(eq + 1);
            bool ok = true;
            if (k == "ptrs") {
                std::istringstream ps(v);
                std::string q;
                while (std::getline(ps, q, ',')) ok = ok && set_ptr(p, q);
            } else if (k == "in_scale") p.in_scale = (float)atof(v.c_str());
            else if (k == "out_scale") p.out_scale = (float)atof(v.c_str());
            else ok = set_int(p, k, atol(v.c_str()));
            if (!ok) { fprintf(stderr, "%s: unknown field in '%s'\n", name.c_str(), tok.c_str()); return 2; }
        }
        if (p.n_cu < 0) p.n_cu = g_ncu;
        g_launches.clear();
        g_attrs.clear();
        const hipError_t e = frp::launch_conv(p, nullptr);
        print_record(name, p, (int)e);
    }
    return 0;
}
