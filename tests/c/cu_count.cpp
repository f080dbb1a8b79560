// Prints the compute-unit count of HIP device 0 (tests/test_tail_plan.py sizes its batch by it).
#include <hip/hip_runtime_api.h>

#include <cstdio>

int main() {
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0) != hipSuccess || cus <= 0) return 1;
  std::printf("%d\n", cus);
  return 0;
}
