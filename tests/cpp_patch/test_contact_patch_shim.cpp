// C++ shim check of the contact-patch API (include/hppfcl_amd_compat.hpp): box on box and box on a halfspace through
// hpp::fcl::computeContactPatch and ComputeContactPatch, against the patches the reference's own tests expect
// (test/contact_patch.cpp: box_box, halfspace_box).  Built with g++ by tests/test_contact_patch_gpu.py; exits 0 on success.
#include <cstdio>

#include "hppfcl_amd_compat.hpp"

using namespace hpp::fcl;

static int check(const char* name, const CollisionGeometry* o1, const Transform3f& tf1, const CollisionGeometry* o2,
                 const Transform3f& tf2, const Vec3f* corners, FCL_REAL sign) {
  CollisionRequest col_req;
  CollisionResult col_res;
  collide(o1, tf1, o2, tf2, col_req, col_res);
  if (!col_res.isCollision()) {
    std::printf("%s: no collision\n", name);
    return 1;
  }
  const ContactPatchRequest req;
  ContactPatchResult res1(req), res2(req);
  computeContactPatch(o1, tf1, o2, tf2, col_res, req, res1);
  ComputeContactPatch(o1, o2)(tf1, tf2, col_res, req, res2);
  if (res1.numContactPatches() != 1 || res2.numContactPatches() != 1) {
    std::printf("%s: %zu / %zu patches\n", name, res1.numContactPatches(), res2.numContactPatches());
    return 1;
  }
  const Contact& c = col_res.getContact(0);
  ContactPatch expected;
  // constructContactPatchFrameFromContact: the frame's normal is what isSame compares; its x / y axes are free
  const Vec3f n = c.normal;
  Matrix3f R;
  const Vec3f u = std::abs(n[0]) > 0.5 ? Vec3f(-n[1], n[0], 0) : Vec3f(0, -n[2], n[1]);
  const Vec3f x = u / u.norm();
  const Vec3f y(n[1] * x[2] - n[2] * x[1], n[2] * x[0] - n[0] * x[2], n[0] * x[1] - n[1] * x[0]);
  for (int i = 0; i < 3; ++i) {
    R(i, 0) = x[i];
    R(i, 1) = y[i];
    R(i, 2) = n[i];
  }
  expected.tf = Transform3f(R, c.pos);
  expected.penetration_depth = c.penetration_depth;
  for (int i = 0; i < 4; ++i) expected.addPoint(corners[i] + n * (sign * c.penetration_depth / 2));
  const bool ok = res1.getContactPatch(0).isSame(expected, 1e-6) && res2.getContactPatch(0).isSame(expected, 1e-6);
  std::printf("%s: %zu points, %s\n", name, res1.getContactPatch(0).size(), ok ? "same" : "DIFFERENT");
  return ok ? 0 : 1;
}

int main() {
  const FCL_REAL h = 0.5, off = 0.001;
  const Box box1(2 * h, 2 * h, 2 * h), box2(2 * h, 2 * h, 2 * h);
  const Transform3f I;
  const Transform3f up(Vec3f(0, 0, 2 * h - off));
  const Vec3f top[4] = {Vec3f(h, h, h), Vec3f(h, -h, h), Vec3f(-h, -h, h), Vec3f(-h, h, h)};
  int bad = check("box_box", &box1, I, &box2, up, top, +1);
  const Halfspace hs(Vec3f(0, 0, 1), 0);
  const Transform3f rest(Vec3f(0, 0, h - off));
  const Vec3f bottom[4] = {rest.transform(Vec3f(h, h, -h)), rest.transform(Vec3f(h, -h, -h)), rest.transform(Vec3f(-h, -h, -h)),
                           rest.transform(Vec3f(-h, h, -h))};
  bad += check("halfspace_box", &hs, I, &box1, rest, bottom, -1);
  return bad == 0 ? 0 : 1;
}
