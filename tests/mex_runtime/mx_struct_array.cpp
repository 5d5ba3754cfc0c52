// Struct ARRAYS for the in-process mx runtime: mx_runtime.cpp keeps one value per field, i.e. 1 x 1 structs (mxSetField / mxGetField refuse an element index
// other than 0).  A host that needs [n x 1] struct arrays links this file with  -Wl,--wrap=mxSetField -Wl,--wrap=mxGetField : element 0 stays where the runtime keeps
// it, elements 1.. live in a side table keyed by (array, element, field).  Documented semantics: mxGetField returns NULL for an unknown field or an unset element.
#include <map>
#include <string>
#include <tuple>

#include "mx_runtime.hpp"

extern "C" {
void __real_mxSetField(mxArray*, mwIndex, const char*, mxArray*);
mxArray* __real_mxGetField(const mxArray*, mwIndex, const char*);
void __wrap_mxSetField(mxArray*, mwIndex, const char*, mxArray*);
mxArray* __wrap_mxGetField(const mxArray*, mwIndex, const char*);
}
namespace {
std::map<std::tuple<const mxArray*, mwIndex, std::string>, mxArray*>& side() { static std::map<std::tuple<const mxArray*, mwIndex, std::string>, mxArray*> m; return m; }
}
void __wrap_mxSetField(mxArray* a, mwIndex i, const char* name, mxArray* v) {
  if (i == 0) { __real_mxSetField(a, 0, name, v); return; }
  if (!mxIsStruct(a) || i >= mxGetNumberOfElements(a)) mexErrMsgIdAndTxt("MATLAB:mxSetField", "element %d of a struct array with %d elements", (int)i, (int)mxGetNumberOfElements(a));
  if (!__real_mxGetField(a, 0, name)) mexErrMsgIdAndTxt("MATLAB:mxSetField", "no such field %s", name);
  mxArray*& slot = side()[std::make_tuple((const mxArray*)a, i, std::string(name))];
  if (slot) mxr_destroy(slot);
  slot = v;
}
mxArray* __wrap_mxGetField(const mxArray* a, mwIndex i, const char* name) {
  if (i == 0) return __real_mxGetField(a, 0, name);
  auto it = side().find(std::make_tuple(a, i, std::string(name)));
  return it == side().end() ? nullptr : it->second;
}
