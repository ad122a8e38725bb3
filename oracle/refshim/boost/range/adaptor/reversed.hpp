// Stand-in for the one Boost facility the reference uses: boost::adaptors::reverse in a range-for.
#pragma once
namespace boost { namespace adaptors {
template <class C> struct reversed_view { C& c; auto begin() { return c.rbegin(); } auto end() { return c.rend(); } };
template <class C> reversed_view<C> reverse(C& c) { return {c}; }
}}
