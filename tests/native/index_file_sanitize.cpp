// Sanitizer driver for the reader and the writer of the index file (test infrastructure; built by tests/test_index_growth_host.py with
// g++ -fsanitize=address,undefined from hesaff_amd/csrc/hostio.cpp + jpeg_decode.cpp).
//   index_file_sanitize <file>...   every file through hesaff_read_index_file.  Any return code is fine: the point is that a
//                                   truncated or corrupt file is refused without touching memory the reader does not own, that a
//                                   refusal hands out no buffer, and that every byte a success promises is readable and obeys the
//                                   rules the reader states.  What was read goes through hesaff_write_index_file to <file>.again
//                                   and must come back array for array.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "../../include/hesaff_amd.h"

struct File {
   int embedded = -1, k = -1, n = -1;
   int64_t keys = -1, postings = -1;
   uint32_t *df = nullptr, *post = nullptr, *kc = nullptr, *ki = nullptr;
   uint64_t *ks = nullptr;
   int read(const char *path) { return hesaff_read_index_file(path, &embedded, &k, &n, &keys, &postings, &df, &post, &kc, &ki, &ks); }
   bool nothing() const { return !df && !post && !kc && !ki && !ks && embedded == 0 && k == 0 && n == 0 && keys == 0 && postings == 0; }
   ~File() { hesaff_free(df); hesaff_free(post); hesaff_free(kc); hesaff_free(ki); hesaff_free(ks); }
};

static bool same(const void *a, const void *b, size_t bytes) { return bytes == 0 || (a && b && memcmp(a, b, bytes) == 0); }

int main(int argc, char **argv)
{
   int whole = 0, refused = 0;
   for (int i = 1; i < argc; i++) {
      File f;
      if (f.read(argv[i]) != HESAFF_OK) {
         if (!f.nothing()) return 3;   // an error must not hand out a buffer
         refused++;
         continue;
      }
      if (f.k < 1 || f.k > (1 << 20) || f.n < 1 || f.n > (1 << 20) || f.keys < 0 || f.keys > ((int64_t)1 << 28) || f.postings < 0 || f.postings > f.keys) return 4;
      if (!f.df || (f.postings > 0) != (f.post != nullptr)) return 5;
      if (f.embedded ? (!f.kc || (f.keys > 0) != (f.ki != nullptr) || (f.keys > 0) != (f.ks != nullptr)) : (f.kc || f.ki || f.ks)) return 6;
      uint64_t sum_df = 0, sum_kc = 0, x = 0;
      for (int w = 0; w < f.k; w++) {
         if (f.df[w] > (uint32_t)f.n) return 7;
         sum_df += f.df[w];
         if (f.embedded) sum_kc += f.kc[w];
      }
      if (sum_df != (uint64_t)f.postings || (f.embedded && sum_kc != (uint64_t)f.keys)) return 8;
      for (int64_t p = 0; p < 2 * f.postings; p++) x += f.post[p];
      if (f.embedded) for (int64_t j = 0; j < f.keys; j++) x += f.ki[j] ^ f.ks[j];
      if (x == 0x0123456789abcdefull) puts("");
      const std::string again = std::string(argv[i]) + ".again";
      if (hesaff_write_index_file(again.c_str(), f.embedded, f.k, f.n, f.keys, f.postings, f.df, f.post, f.kc, f.ki, f.ks) != HESAFF_OK) return 9;
      File g;
      if (g.read(again.c_str()) != HESAFF_OK) return 10;
      if (g.embedded != f.embedded || g.k != f.k || g.n != f.n || g.keys != f.keys || g.postings != f.postings) return 11;
      if (!same(f.df, g.df, (size_t)f.k * 4) || !same(f.post, g.post, (size_t)f.postings * 8)) return 12;
      if (f.embedded && (!same(f.kc, g.kc, (size_t)f.k * 4) || !same(f.ki, g.ki, (size_t)f.keys * 4) || !same(f.ks, g.ks, (size_t)f.keys * 8))) return 13;
      remove(again.c_str());
      whole++;
   }
   printf("read whole=%d refused=%d\n", whole, refused);
   return 0;
}
