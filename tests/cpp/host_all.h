// The host side of libmtr.so as one translation unit, for the CPU harnesses of this directory: every csrc/host_*.cpp.
// A file missing here shows up as an undefined symbol when a harness links.
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
#include "../../mt_renderer_amd/csrc/host_frame.cpp"
#include "../../mt_renderer_amd/csrc/host_submit.cpp"
#include "../../mt_renderer_amd/csrc/host_shard.cpp"
