// Stand-alone driver of the host-only part of the C ABI (monohair_amd/csrc/capi_host.cpp), built with sanitizers by
// tests/test_capi_host_sanitized.py.  It reads the inputs the test wrote into the working directory (<name>.bin, raw arrays),
// calls the library and writes what came back; every expected value is worked out by the test, none here.
//   capi_host_main all      every case          capi_host_main threads      the two threaded-writer runs only
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../include/mh_pmvo.h"

template <class T>
static std::vector<T> load(const std::string &name) {
    std::ifstream f(name + ".bin", std::ios::binary);
    if (!f) {
        fprintf(stderr, "missing input %s.bin\n", name.c_str());
        exit(2);
    }
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<T> v(raw.size() / sizeof(T));
    if (!v.empty()) memcpy(v.data(), raw.data(), v.size() * sizeof(T));
    return v;
}

template <class T>
static void save(const std::string &name, const std::vector<T> &v) {
    std::ofstream f(name + ".bin", std::ios::binary);
    f.write((const char *)v.data(), (std::streamsize)(v.size() * sizeof(T)));
}

static FILE *g_status;
static void status(const char *key, int rc) { fprintf(g_status, "%s %d\n", key, rc); }

static void copy_file(const char *from, const std::string &to) {
    std::ifstream in(from, std::ios::binary);
    std::ofstream out(to + ".bin", std::ios::binary);
    out << in.rdbuf();
}

static void writer_threads(const std::vector<char> &prefix) {
    const auto idx = load<long long>("big_idx");
    const auto val = load<double>("big_val");
    const size_t nelem = (size_t)load<long long>("big_nelem")[0];
    status("ws_t1", mh_mat_write_sparse("ws_t1.mat", prefix.data(), prefix.size(), nelem * 8, idx.data(), val.data(), idx.size(), 1));
    status("ws_t4", mh_mat_write_sparse("ws_t4.mat", prefix.data(), prefix.size(), nelem * 8, idx.data(), val.data(), idx.size(), 4));
}

static void writer_cases(const std::vector<char> &prefix) {
    const auto idx = load<long long>("small_idx");
    const auto val = load<double>("small_val");
    const size_t nelem = (size_t)load<long long>("small_nelem")[0];
    status("ws_small", mh_mat_write_sparse("ws_small.mat", prefix.data(), prefix.size(), nelem * 8, idx.data(), val.data(), idx.size(), 1));
    status("ws_empty", mh_mat_write_sparse("ws_empty.mat", prefix.data(), prefix.size(), nelem * 8, nullptr, nullptr, 0, 1));
    const long long past = (long long)nelem;
    const double one = 1.0;
    status("ws_range", mh_mat_write_sparse("ws_range.mat", prefix.data(), prefix.size(), nelem * 8, &past, &one, 1, 1));
    fprintf(g_status, "ws_range_error %s\n", mh_last_error());
}

static void handle_cases(const std::vector<char> &prefix) {
    const auto dims = load<long long>("grid_dims");      // X, Y, Z
    const int X = (int)dims[0], Y = (int)dims[1], Z = (int)dims[2];
    const size_t plane = (size_t)X * Y * Z;
    const auto vox = load<long long>("vox");
    const auto touch = load<long long>("touch_idx");
    const auto sidx = load<long long>("store_idx");
    const auto sval = load<double>("store_val");
    const auto ori32 = load<float>("ori32");
    const auto ori64 = load<double>("ori64");
    const auto bad_vox = load<long long>("bad_vox");

    void *h = (void *)&h;      // (anything but NULL: a failed open must clear it)
    status("open_prefix4", mh_mat_sparse_open("sp_bad.mat", prefix.data(), 4, plane * 8, &h));
    status("open_prefix4_handle_null", h == nullptr);
    status("close_null", mh_mat_sparse_close(nullptr));

    status("occ_open", mh_mat_sparse_open("sp_occ.mat", prefix.data(), prefix.size(), plane * 8, &h));
    status("occ_touch", mh_mat_sparse_touch(h, touch.data(), touch.size()));
    copy_file("sp_occ.mat", "sp_occ_after_touch");
    status("occ_store", mh_mat_sparse_store(h, sidx.data(), sval.data(), sidx.size()));
    status("occ_store_voxels", mh_mat_sparse_store_voxels(h, vox.data(), nullptr, 0, vox.size() / 3, X, Y, Z));
    status("occ_close", mh_mat_sparse_close(h));

    status("ori32_open", mh_mat_sparse_open("sp_ori32.mat", prefix.data(), prefix.size(), plane * 24, &h));
    status("ori32_touch", mh_mat_sparse_touch(h, touch.data(), touch.size()));
    status("ori32_bad_voxel", mh_mat_sparse_store_voxels(h, bad_vox.data(), ori32.data(), 0, bad_vox.size() / 3, X, Y, Z));
    status("ori32_store_voxels", mh_mat_sparse_store_voxels(h, vox.data(), ori32.data(), 0, vox.size() / 3, X, Y, Z));
    status("ori32_close", mh_mat_sparse_close(h));

    status("ori64_open", mh_mat_sparse_open("sp_ori64.mat", prefix.data(), prefix.size(), plane * 24, &h));
    status("ori64_store_voxels", mh_mat_sparse_store_voxels(h, vox.data(), ori64.data(), 1, vox.size() / 3, X, Y, Z));
    status("ori64_close", mh_mat_sparse_close(h));
}

// the inputs <tag>_{flag,pts,first,len,seeds}; n < 0: as many strands as `len` holds
static void accept_case(const std::string &tag, const std::string &out, int stride, int mode, int n) {
    const auto whz = load<long long>("accept_whz");
    auto flag = load<float>(tag + "_flag");
    const auto pts = load<float>(tag + "_pts");
    const auto first = load<int32_t>(tag + "_first");
    const auto len = load<int32_t>(tag + "_len");
    const auto seeds = load<float>(tag + "_seeds");
    if (n < 0) n = (int)len.size();
    std::vector<uint8_t> accepted(len.size(), 7);
    status(out.c_str(), mh_strands_accept((int)whz[0], (int)whz[1], (int)whz[2], flag.data(), pts.data(), first.data(),
                                          len.data(), stride, seeds.data(), n, mode, accepted.data()));
    save(out + "_flag_out", flag);
    save(out + "_accepted", accepted);
}

int main(int argc, char **argv) {
    const std::string what = argc > 1 ? argv[1] : "all";
    g_status = fopen("status.txt", "w");
    if (!g_status) return 2;
    const auto prefix = load<char>("prefix");
    writer_threads(prefix);
    if (what == "all") {
        writer_cases(prefix);
        handle_cases(prefix);
        const int stride = (int)load<long long>("accept_stride")[0];
        accept_case("acc0", "acc0", stride, 0, -1);
        accept_case("acc1", "acc1", stride, 1, -1);
        accept_case("acc0", "acc_none", stride, 0, 0);
    }
    fclose(g_status);
    return 0;
}
