// P/Invoke surface of libsnappier_hip_layout.so -- one declaration per function of include/snappier_hip_layout.h, same order.
// That library is linked against libsnappier_hip.so and takes its contexts (NativeMethods.snp_ctx_create).
using System;
using System.Runtime.InteropServices;

namespace Snappier.Gpu;

internal static unsafe class NativeMethodsLayout
{
    private const string Lib = "snappier_hip_layout";                           // libsnappier_hip_layout.so
    private const CallingConvention Cc = CallingConvention.Cdecl;

    // ---- batch, device pointers (asynchronous on the context's stream): decoded lengths and the output layout of a decode call
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_decompress_layout_workspace(uint nbuffers);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_decompress_layout_batch(IntPtr ctx, IntPtr dIn, IntPtr dInOff, IntPtr dInLen, uint nbuffers, uint align, ulong arenaCap, IntPtr dOutOff, IntPtr dOutCap, IntPtr dDeclared, IntPtr dStatus, IntPtr dWork, IntPtr dResult);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_frame_decode_layout_workspace(uint nstreams, uint maxSpans);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_frame_decode_layout_batch(IntPtr ctx, IntPtr dIn, IntPtr dInOff, IntPtr dInLen, uint nstreams, uint maxSpans, uint align, ulong arenaCap, IntPtr dOutOff, IntPtr dOutCap, IntPtr dDecodedLen, IntPtr dNchunks, IntPtr dStatus, IntPtr dWork, IntPtr dResult);
}
