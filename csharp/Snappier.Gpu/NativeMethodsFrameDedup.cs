// P/Invoke surface of libsnappier_hip_frame_dedup.so -- one declaration per function of include/snappier_hip_frame_dedup.h, same order.
// That library is linked against libsnappier_hip.so and takes its contexts (NativeMethods.snp_ctx_create).
using System;
using System.Runtime.InteropServices;

namespace Snappier.Gpu;

internal static unsafe class NativeMethodsFrameDedup
{
    private const string Lib = "snappier_hip_frame_dedup";                      // libsnappier_hip_frame_dedup.so
    private const CallingConvention Cc = CallingConvention.Cdecl;

    internal const ulong SnpDedupNone = ulong.MaxValue;                         // SNP_DEDUP_NONE: canon of a row that takes no part

    // ---- batch, device pointers (asynchronous on the context's stream): the streams and their index as
    // NativeMethodsFrameIndex.snp_frame_read_indexed_batch takes them, the first nbase of them the base -> the pack (dOut, dOutLen[1]) and its
    // index (dPkFirst[2], dPkStart / dPkPos maxEntries rows, dPkTotal[1], dPkTail[1]), dCanon (nentries), dStatus (nstreams) and the recipes in
    // the form NativeMethodsFrameCompose.snp_frame_compose_indexed_batch takes (dSegFirst nstreams - nbase + 1 values, the others maxSegs);
    // dResult holds 8 values
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_frame_dedup_indexed_workspace(uint nstreams, ulong nentries);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_frame_dedup_indexed_batch(IntPtr ctx, IntPtr dIn, IntPtr dInOff, IntPtr dInLen, uint nstreams, IntPtr dIdxFirst, IntPtr dIdxStart, IntPtr dIdxPos, IntPtr dIdxTotal, IntPtr dIdxTail, ulong nentries, uint nbase, uint maxEntries, uint maxSegs, ulong outCap, IntPtr dOut, IntPtr dOutLen, IntPtr dStatus, IntPtr dCanon, IntPtr dPkFirst, IntPtr dPkStart, IntPtr dPkPos, IntPtr dPkTotal, IntPtr dPkTail, IntPtr dSegFirst, IntPtr dSegStream, IntPtr dSegOff, IntPtr dSegLen, IntPtr dWork, IntPtr dResult);
}
