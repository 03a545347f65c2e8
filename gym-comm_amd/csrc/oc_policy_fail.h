// oc_policy_fail.h -- the one last-error text of liboc_policy.so, for both of its translation units.
// Not exported.
#ifndef OC_POLICY_FAIL_H
#define OC_POLICY_FAIL_H
namespace ocpol {
// formats what oc_policy_last_error() returns (oc_policy.hip owns the buffer); returns -1
int fail(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
}
#endif
