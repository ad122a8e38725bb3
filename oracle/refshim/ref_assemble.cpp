// ref_assemble -- TEST INFRASTRUCTURE ONLY: the reference's analyze_bristol + assemble_bristol on one file.
//
//   ref_assemble <circuit.txt> <new_flag 0|1> <debug_flag 0|1>
//
// The reference names its own output: <path up to the first '.'>_FHE.out, next to the input.
#include <cstdint>
#include <cstdlib>
#include <iostream>

#include "analyze.h"
#include "assemble.h"

int main(int argc, char** argv) {
    if (argc != 4) {
        std::cerr << "usage: ref_assemble <circuit.txt> <new_flag> <debug_flag>" << std::endl;
        return 2;
    }
    Analysis a = analyze_bristol(argv[1], false, std::atoi(argv[2]) != 0);
    assemble_bristol(a, 0, std::atoi(argv[3]) != 0);
    return 0;
}
