// The switch table's rows, its parsers, the one environment read of csrc/, and the host queries over it (no device).
#include <cstdlib>
#include <mutex>
#include "common.h"
#include "kernels.h"

namespace dvsr {
namespace {

enum class Parser { OFF0, ON1, INT, SET, UP2, DCN_FWD, DCN_BWD };
struct Row { const char* env; int scope; Parser parser; int dflt; const char* doc; };
const Row rows[] = {
#define X(name, scope, parser, dflt, doc) {"DVSR_" #name, DVSR_SW_##scope, Parser::parser, dflt, doc},
    DVSR_SWITCHES(X)
#undef X
};

int parse(const Row& r, const char* v) {
  if (!v) return r.dflt;
  switch (r.parser) {
    case Parser::OFF0: return v[0] != '0';
    case Parser::ON1: return v[0] == '1';
    case Parser::INT: return atoi(v);
    case Parser::SET: return 1;
    case Parser::UP2: return v[0] == '4';
    case Parser::DCN_FWD: return (!v[0] || v[0] == 's') ? 3 : (v[0] == 'r' ? 2 : 0);   // ('lds', retired in round 6, is the DMA kernel)
    case Parser::DCN_BWD: return v[0] == 'u' ? 1 : (v[0] == 'f' ? 2 : 0);
  }
  return r.dflt;
}

}  // namespace

SwKept sw_kept[(int)Sw::COUNT];

int sw_read(Sw s) {
  const Row& r = rows[(int)s];
  if (r.scope != DVSR_SW_PROCESS) return parse(r, getenv(r.env));
  static std::mutex mu;   // (two threads at a first read: the first one's answer is everybody's)
  std::lock_guard<std::mutex> lock(mu);
  SwKept& k = sw_kept[(int)s];
  if (!k.known.load(std::memory_order_relaxed)) {
    k.value = parse(r, getenv(r.env));
    k.known.store(true, std::memory_order_release);
  }
  return k.value;
}

}  // namespace dvsr

using namespace dvsr;

extern "C" int dvsr_switch_count(void) { return (int)Sw::COUNT; }

static bool is_switch(int i) { return i >= 0 && i < (int)Sw::COUNT; }

extern "C" int dvsr_switch_info(int i, const char** name, int* scope, int* dflt, const char** doc) {
  DVSR_REQUIRE(is_switch(i), DVSR_ERR_INVALID, "switch_info: switch %d of %d", i, (int)Sw::COUNT);
  const Row& r = rows[i];
  if (name) *name = r.env;
  if (scope) *scope = r.scope;
  if (dflt) *dflt = r.dflt;
  if (doc) *doc = r.doc;
  return DVSR_OK;
}

extern "C" int dvsr_switch_parse(int i, const char* text, int* value) {
  DVSR_REQUIRE(is_switch(i) && value, DVSR_ERR_INVALID, "switch_parse: switch %d of %d, value %p", i, (int)Sw::COUNT, (void*)value);
  *value = parse(rows[i], text);
  return DVSR_OK;
}

extern "C" int dvsr_switch_value(int i, int* value) {
  DVSR_REQUIRE(is_switch(i) && value, DVSR_ERR_INVALID, "switch_value: switch %d of %d, value %p", i, (int)Sw::COUNT, (void*)value);
  *value = sw((Sw)i);
  return DVSR_OK;
}
