// Sanitizer driver for the two readers of Hamming embedding (test infrastructure; built by tests/test_embedding_sanitize.py with
// g++ -fsanitize=address,undefined from hesaff_amd/csrc/hostio.cpp + jpeg_decode.cpp).
//   embedding_files_sanitize <file>...   every file through hesaff_read_embedding and hesaff_read_signatures.  Any return code is
//                                        fine: the point is that a truncated or corrupt file is refused without touching memory the
//                                        reader does not own, that a refusal hands out no buffer, and that every byte a success
//                                        promises is readable and obeys the format's rules.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../../include/hesaff_amd.h"

int main(int argc, char **argv)
{
   int embeddings = 0, signatures = 0, refused = 0;
   for (int i = 1; i < argc; i++) {
      int8_t *P = nullptr;
      int32_t *tau = nullptr;
      int k = -1;
      const int rc = hesaff_read_embedding(argv[i], &P, &tau, &k);
      if (rc == HESAFF_OK) {
         if (!P || !tau || k < 1 || k > (1 << 20)) return 3;
         long long sum = 0;
         for (int e = 0; e < 64 * 128; e++) {
            if (P[e] == -128) return 4;   // the reader refuses what hesaff_set_embedding would
            sum += P[e];
         }
         for (long long e = 0; e < (long long)k * 64; e++) sum += tau[e];
         if (sum == 0x7fffffffffffffffll) puts("");
         hesaff_free(P); hesaff_free(tau);
         embeddings++;
      } else {
         if (P || tau || k != 0) return 5;   // an error must not hand out a buffer
         refused++;
      }
      uint64_t *sigs = nullptr;
      int count = -1;
      const int rs = hesaff_read_signatures(argv[i], &sigs, &count);
      if (rs == HESAFF_OK) {
         if (count < 0 || (count > 0) != (sigs != nullptr)) return 6;
         uint64_t x = 0;
         for (int e = 0; e < count; e++) x ^= sigs[e];
         if (x == 0x0123456789abcdefull) puts("");
         if (hesaff_signatures_is_complete(argv[i]) != count) return 7;
         hesaff_free(sigs);
         signatures++;
      } else {
         if (sigs || count != 0) return 8;
         if (hesaff_signatures_is_complete(argv[i]) != -1) return 9;
         refused++;
      }
   }
   printf("read embeddings=%d signatures=%d refused=%d\n", embeddings, signatures, refused);
   return 0;
}
