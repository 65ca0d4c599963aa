// The C boundary (include/tts_hip.h): the last-error slot and the one catch ladder every
// extern "C" entry runs under, so no C++ exception leaves the library.
#pragma once
#include <mutex>
#include <new>

#include "runtime.h"

namespace tts {

// tts_last_error()'s thread-local text (engine.cpp)
void set_last_error(const char* msg);

// the first ctl_size bytes of a caller's tts_prosody (an older header's shorter struct: the
// missing controls neutral) -> the kernels' struct (engine.cpp); false: not a size this library reads
struct VarianceCtl;
bool read_prosody(const tts_prosody* ctl, size_t ctl_size, VarianceCtl* out);

// entries without an engine: f() under the ladder
template <typename F>
int guarded(F&& f) {
  try {
    f();
    return TTS_OK;
  } catch (const TtsError& e) {
    set_last_error(e.what());
    return e.code;
  } catch (const std::bad_alloc&) {
    set_last_error("out of host memory");
    return TTS_ERR_NOMEM;
  } catch (const std::exception& e) {
    set_last_error(e.what());
    return TTS_ERR_INVALID;
  }
}

// entries on an engine: also takes its mutex and selects its device
template <typename E, typename F>
int guarded(E* eng, F&& f) {
  return guarded([&] {
    if (!eng) throw TtsError(TTS_ERR_INVALID, "null engine");
    std::lock_guard<std::mutex> lk(eng->mu);
    HIP_CHECK(hipSetDevice(eng->device));
    f();
  });
}

}  // namespace tts
