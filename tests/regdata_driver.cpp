// Runs smcn_regdata.hpp over the cases of a text file and prints what it computes (tests/test_regdata_host.py builds this
// with the address and undefined-behaviour sanitizers).  Every block lives in a heap array of exactly its length, so a read
// past a caller-supplied length is a sanitizer error.
//
// input, one case per line:   <name> <model id> <n doubles> <block ..> [<n doubles> <new rows' block ..>]
// output per case:            case <name> / msg <check message> / ints <RegLayout's integers> / vec <repacked image>
//   and, with new rows:       splice <message> / full <spliced block> / then msg, ints, vec of the spliced block
// doubles are hex floats on both sides; ints and vec follow an accepted block only.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>

#include "smcn_regdata.hpp"

using smcn::RegLayout;

static void print_doubles(const char* tag, const double* v, size_t n) {
    std::printf("%s %zu", tag, n);
    for (size_t i = 0; i < n; ++i) std::printf(" %a", v[i]);
    std::printf("\n");
}

// msg / ints / vec of one block; true if it was accepted
static bool check_and_repack(int model, const double* block, int64_t len, RegLayout* L) {
    const std::string msg = smcn::reg_check(model, block, len, L);
    std::printf("msg %s\n", msg.c_str());
    if (!msg.empty()) return false;
    std::printf("ints %d %d %d %lld %lld %lld %d %d %d %lld %lld %lld %lld %lld %lld %lld %lld %d %d %lld %lld\n", L->model,
                L->fam, L->K, (long long)L->n, (long long)L->p, (long long)L->J, L->ic, L->Dc, L->D, (long long)L->nh,
                (long long)L->npri, (long long)L->y0, (long long)L->g0, (long long)L->X0, (long long)L->len,
                (long long)L->t0, (long long)L->rows, L->RS, L->ys, (long long)L->c0, (long long)L->rlen);
    std::vector<double> mup;
    smcn::reg_repack(*L, block, mup);
    print_doubles("vec", mup.data(), mup.size());
    return true;
}

static std::unique_ptr<double[]> read_block(std::istringstream& in, int64_t* len) {
    *len = -1;
    in >> *len;
    if (*len < 0) return nullptr;
    std::unique_ptr<double[]> b(new double[*len]);
    std::string tok;
    for (int64_t i = 0; i < *len; ++i) {
        in >> tok;
        b[i] = std::strtod(tok.c_str(), nullptr);
    }
    return b;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream f(argv[1]);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string name;
        int model = 0;
        int64_t len = 0, len2 = 0;
        in >> name >> model;
        const std::unique_ptr<double[]> block = read_block(in, &len);
        if (!block || !in) return 3;
        const std::unique_ptr<double[]> rows = read_block(in, &len2);      // (none: a check-only case)
        std::printf("case %s\n", name.c_str());
        RegLayout L, L2;
        if (!check_and_repack(model, block.get(), len, &L) || !rows) continue;
        std::vector<double> full;
        const std::string why = smcn::reg_splice(L, block.get(), rows.get(), len2, full);
        std::printf("splice %s\n", why.c_str());
        if (!why.empty()) continue;
        print_doubles("full", full.data(), full.size());
        check_and_repack(model, full.data(), (int64_t)full.size(), &L2);
    }
    return 0;
}
