// The option table of options.h: the one reader of the environment, and msml_set_option / msml_get_option /
// msml_option_name (msml_hip.h).
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "options.h"

namespace {
enum Kind { PRESENT, INT, LONG, NOT0, NOT0CH };

long parse(Kind kind, const char* text, long def) {
  if (!text) return def;
  switch (kind) {
    case PRESENT: return 1;
    case INT: return atoi(text);
    case LONG: return atol(text);
    case NOT0: return atoi(text) != 0;
    default: return text[0] != '0';
  }
}

struct Entry {
  const char* name;
  MsmlOption MsmlOptions::*field;
};
const Entry kTable[] = {
#define X(field, env, kind, def) {env, &MsmlOptions::field},
    MSML_OPTIONS(X)
#undef X
};
const int kCount = sizeof(kTable) / sizeof(kTable[0]);

MsmlOptions& table() {
  static MsmlOptions opt;
  static const bool filled = [] {
#define X(field, env, kind, def) opt.field.v.store(parse(kind, getenv(env), def), std::memory_order_relaxed);
    MSML_OPTIONS(X)
#undef X
    return true;
  }();
  (void)filled;
  return opt;
}

MsmlOption* find(const char* name) {
  for (int i = 0; i < kCount; i++)
    if (strcmp(kTable[i].name, name) == 0) return &(table().*kTable[i].field);
  msml_set_error("unknown option %s", name);
  return nullptr;
}
}  // namespace

const MsmlOptions& msml_opt() { return table(); }

extern "C" int msml_set_option(const char* name, long value) {
  MSML_CHECK(name, MSML_ERR_SHAPE, "msml_set_option: null name");
  MsmlOption* o = find(name);
  if (!o) return MSML_ERR_UNSUPPORTED;
  o->v.store(value, std::memory_order_relaxed);
  return MSML_OK;
}

extern "C" int msml_get_option(const char* name, long* value) {
  MSML_CHECK(name && value, MSML_ERR_SHAPE, "msml_get_option: null pointer");
  const MsmlOption* o = find(name);
  if (!o) return MSML_ERR_UNSUPPORTED;
  *value = *o;
  return MSML_OK;
}

extern "C" const char* msml_option_name(int index) { return index >= 0 && index < kCount ? kTable[index].name : nullptr; }
