// ref_run -- TEST INFRASTRUCTURE ONLY: a driver of ours over the reference's public Circuit API
// (ReadFile, Reset, setPlaintext / setEncrypted / setVerify, SetInput, Clock), compiled against the reference's
// unmodified sources and oracle/refshim/binfhecontext.h.
//
//   ref_run <circuit.out> <TOY|STD128_OPT> <GINX|AP> <plain|enc|verify> <vector> [<vector> ...]
//
// A vector is the input buses joined by ',', each bus a string of 0/1 with bit 0 FIRST ("10,11" = In1 bits {1,0}, In2
// bits {1,1}).  Every vector is one Reset / SetInput / Clock; vector k (from 0) encrypts from stream index
// (k + 2) << 44: the engine's Circuit counts the Reset that ReadFile makes, so the caller's k-th Reset (from 0) is its
// epoch k + 2 (see binfhecontext.h).  After each Clock one line
// "OUT <bits, bit 0 first>" goes to stdout (the reference's own progress lines are there too) and "M vector k" /
// "M clock k" / "M done k" markers go to the trace.
#include <cstring>
#include <iostream>
#include <string>

#include "circuit.h"

int main(int argc, char** argv) {
    if (argc < 6) {
        std::cerr << "usage: ref_run <circuit.out> <TOY|STD128_OPT> <GINX|AP> <plain|enc|verify> <vector>..." << std::endl;
        return 2;
    }
    const std::string set_s = argv[2], method_s = argv[3], mode = argv[4];
    if ((set_s != "TOY" && set_s != "STD128_OPT") || (method_s != "GINX" && method_s != "AP") ||
        (mode != "plain" && mode != "enc" && mode != "verify")) {
        std::cerr << "ref_run: bad parameter set, method or mode" << std::endl;
        return 2;
    }
    Circuit circ(set_s == "TOY" ? lbcrypto::TOY : lbcrypto::STD128_OPT, method_s == "AP" ? lbcrypto::AP : lbcrypto::GINX);
    if (!circ.ReadFile(argv[1])) return 1;
    for (int k = 5; k < argc; ++k) {
        Inputs in(1);
        for (const char* p = argv[k]; *p; ++p) {
            if (*p == ',') in.emplace_back();
            else if (*p == '0' || *p == '1') in.back().push_back(*p - '0');
            else { std::cerr << "ref_run: bad vector " << argv[k] << std::endl; return 2; }
        }
        const std::string tag = std::to_string(k - 5);
        circ.Reset();
        circ.setPlaintext(mode == "plain");
        circ.setEncrypted(mode != "plain");
        circ.setVerify(mode == "verify");
        lbcrypto::refshim_set_encrypt_index((uint64_t)(k - 3) << 44);
        lbcrypto::refshim_mark("vector " + tag);
        circ.SetInput(in);
        lbcrypto::refshim_mark("clock " + tag);
        Outputs out = circ.Clock();
        lbcrypto::refshim_mark("done " + tag);
        std::cout << std::endl << "OUT ";
        for (unsigned b : out[0]) std::cout << b;
        std::cout << std::endl;
    }
    return 0;
}
