// The host side of libmtr.so as one translation unit: every csrc/host_*.cpp, as csrc/Makefile picks them up.  Every
// host-side program of this directory includes it, through harness.h.  tests/test_cpp_harness.py holds this list to the
// files that exist: a file missing here goes unnoticed by every program that does not call its entry points.
#pragma once
#include "../../mt_renderer_amd/csrc/host_device.cpp"
#include "../../mt_renderer_amd/csrc/host_texture.cpp"
#include "../../mt_renderer_amd/csrc/host_model.cpp"
#include "../../mt_renderer_amd/csrc/host_anim.cpp"
#include "../../mt_renderer_amd/csrc/host_batch.cpp"
#include "../../mt_renderer_amd/csrc/host_player.cpp"
#include "../../mt_renderer_amd/csrc/host_ctrl.cpp"
#include "../../mt_renderer_amd/csrc/host_events.cpp"
#include "../../mt_renderer_amd/csrc/host_blend.cpp"
#include "../../mt_renderer_amd/csrc/host_spring.cpp"
#include "../../mt_renderer_amd/csrc/host_match.cpp"
#include "../../mt_renderer_amd/csrc/host_frame.cpp"
#include "../../mt_renderer_amd/csrc/host_submit.cpp"
#include "../../mt_renderer_amd/csrc/host_shard.cpp"
