// ens.hip - one n_para's instantiation of the ensemble kernel (compile with -DSMCMI_ENS_D=<1..10>; see enskernel.hpp).
#ifndef SMCMI_ENS_D
#error "compile with -DSMCMI_ENS_D=<n_para>"
#endif
#define SMCMI_INST_UNIT 1               // (the engines' non-template kernels belong to smcmi.hip: kernels.hpp)
#include "enskernel.hpp"
