// Replica groups (group_args.h, engine.hip agbnp_hip_execute_group): the launches that several contexts share.  The kernel
// bodies are those of pair_kernels.hip and tree_kernels.hip; their group entry points are compiled in this translation unit of
// their own, so that the kernels of those two files -- and the compiler's inlining decisions for them -- stay what they are.
#define AGBNP_GROUP_TU
#include "pair_kernels.hip"
#include "tree_kernels.hip"
