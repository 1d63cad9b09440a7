// Image groups of a batch as run_keypoint_stages forms them (hesaff_amd/csrc/batch_plan.h: form_groups), for the per-image Hessian
// counts given as arguments and no large-window rows: prints one line "lo hi" per group.  Built and run by
// tests/test_descriptor_chain.py, which has to know that its batch makes the three patch slots wrap.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../hesaff_amd/csrc/batch_plan.h"

using namespace hesaff_plan;

int main(int argc, char **argv)
{
   const int B = argc - 1;
   std::vector<int32_t> hs(B + 1, 0);
   for (int b = 0; b < B; b++) hs[b + 1] = hs[b] + atoi(argv[b + 1]);
   const std::vector<uint32_t> lrows(B + 1, 0u);
   const GroupPlan p = form_groups(hs.data(), lrows.data(), B, 4u << 20);
   for (const ImageGroup &g : p.groups) printf("%u %u\n", g.lo, g.hi);
   return 0;
}
